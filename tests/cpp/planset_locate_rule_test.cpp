// The plan-set addition to the locate rule (slime_amd/csrc/locate_rule.hpp,
// set_slot / Column::slot_in_set) on the CPU, against a brute-force statement
// written from the header's text (include/slime_rs.h, "plan-set locate"):
//   a clean column is clean; an object whose plan has fewer than two rows
//   reports every mismatching column at slot k + max_rows; otherwise exactly one
//   mismatching row i is slot k + i, exactly one input j satisfying the relation
//   in every row is slot j, and anything else is slot k + max_rows.  Slots
//   k + rows .. k + max_rows - 1 are never named.
// Plans are the first `rows` parity rows of 3/5, 4/6 and 8/12 (rows 1 ... all)
// under every max_rows from max(rows, 2) to rows + 3; per plan: every
// single-shard error, aliases, and 2 x 10^4 random syndromes and double errors.
//   planset_locate_rule_test --cases prints planted cases for
//   tests/planset_locate_ref.py: "rows k max_rows | coefficients | inputs |
//   stored | slot" per line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
#include "locate_rule.hpp"
#include "rs_matrix.hpp"

using namespace slime;

namespace {

typedef unsigned __int128 u128;

struct Code {
  uint32_t k, rows;
  std::vector<uint32_t> c;  // rows x k
  const uint32_t* row(uint32_t i) const { return c.data() + (size_t)i * k; }
};

Code parity_code(int need, int total, int rows) {
  Matrix m;
  if (parity_matrix(need, total - need, &m) != Status::Ok) {
    printf("parity_matrix(%d, %d) failed\n", need, total - need);
    exit(1);
  }
  Code code{(uint32_t)need, (uint32_t)rows, {}};
  for (int i = need; i < need + rows; ++i) code.c.insert(code.c.end(), m.row(i), m.row(i) + need);
  return code;
}

uint32_t dot(const Code& code, uint32_t i, const std::vector<uint32_t>& x) {
  u128 s = 0;
  for (uint32_t j = 0; j < code.k; ++j) s += (u128)code.row(i)[j] * x[j];
  return (uint32_t)(s % kP);
}

// As the device runs it: rows fed one at a time, then both spellings of the set's slot.
uint32_t rule(const Code& code, const std::vector<uint32_t>& x, const std::vector<uint32_t>& stored, uint32_t max_rows,
              bool* agree) {
  locate::Column col;
  col.begin(code.k);
  for (uint32_t i = 0; i < code.rows; ++i) col.row(i, dot(code, i, x), stored[i], code.row(0), code.row(i));
  const uint32_t a = col.slot_in_set(code.k, code.rows, max_rows);
  const uint32_t b = locate::set_slot(col.slot(code.k, code.rows), code.k, code.rows, max_rows);
  *agree = a == b;
  return a;
}

// The statement, with per-row arrays and 128-bit products.
uint32_t brute(const Code& code, const std::vector<uint32_t>& x, const std::vector<uint32_t>& stored, uint32_t max_rows) {
  std::vector<uint64_t> s(code.rows);
  uint32_t nd = 0, last = 0;
  for (uint32_t i = 0; i < code.rows; ++i) {
    const uint32_t comp = dot(code, i, x);
    if (stored[i] != comp) {
      ++nd;
      last = i;
    }
    s[i] = ((uint64_t)(stored[i] % kP) + kP - comp) % kP;
  }
  if (nd == 0) return locate::kNoSlot;
  if (code.rows < 2) return code.k + max_rows;
  if (nd == 1) return code.k + last;
  uint32_t found = 0, which = 0;
  for (uint32_t j = 0; j < code.k && s[0] != 0; ++j) {
    bool ok = true;
    for (uint32_t i = 0; i < code.rows; ++i)
      ok = ok && (u128)s[i] * (code.row(0)[j] % kP) % kP == (u128)s[0] * (code.row(i)[j] % kP) % kP;
    if (ok) {
      ++found;
      which = j;
    }
  }
  return found == 1 ? which : code.k + max_rows;
}

int failures = 0;
bool print_cases = false;
uint64_t checked = 0;

void check(const char* what, const Code& code, const std::vector<uint32_t>& x, const std::vector<uint32_t>& stored,
           uint32_t max_rows, bool keep, const uint32_t* planted = nullptr) {
  bool agree = false;
  const uint32_t got = rule(code, x, stored, max_rows, &agree), ref = brute(code, x, stored, max_rows);
  ++checked;
  bool bad = got != ref || !agree || (planted && got != *planted);
  // never a slot past the plan's own rows, except `unlocated`
  if (got != locate::kNoSlot && got >= code.k + code.rows && got != code.k + max_rows) bad = true;
  if (bad && ++failures <= 10)
    printf("FAIL %s (k %u rows %u max_rows %u): rule %u, brute force %u, planted %d\n", what, code.k, code.rows, max_rows,
           got, ref, planted ? (int)*planted : -2);
  if (keep && print_cases) {
    printf("%u %u %u |", code.rows, code.k, max_rows);
    for (uint32_t v : code.c) printf(" %u", v);
    printf(" |");
    for (uint32_t v : x) printf(" %u", v);
    printf(" |");
    for (uint32_t v : stored) printf(" %u", v);
    printf(" | %u\n", got);
  }
}

void run(const Code& code, uint32_t max_rows, uint64_t seed) {
  std::mt19937_64 rng(seed);
  auto word = [&]() { return (uint32_t)(rng() % kP); };
  const uint32_t k = code.k, rows = code.rows, unl = k + max_rows;
  std::vector<uint32_t> x(k), st(rows);
  for (uint32_t j = 0; j < k; ++j) x[j] = word();
  auto clean = [&]() {
    for (uint32_t i = 0; i < rows; ++i) st[i] = dot(code, i, x);
  };
  clean();
  check("clean", code, x, st, max_rows, true, &locate::kNoSlot);
  const uint32_t deltas[] = {1, 4, kP - 1, 1u << 31, word() | 1u};
  // one wrong input: named when the plan can (rows >= 2), unlocated when it has one row
  for (uint32_t j = 0; j < k; ++j)
    for (uint32_t d : deltas) {
      clean();
      std::vector<uint32_t> y = x;
      y[j] = (uint32_t)(((uint64_t)x[j] + d % kP) % kP);
      if (y[j] == x[j]) continue;
      const uint32_t want = rows < 2 ? unl : j;
      check("input", code, y, st, max_rows, true, &want);
    }
  // one wrong row: its own slot, or unlocated under a one-row plan; stored t + p is wrong too
  for (uint32_t i = 0; i < rows; ++i)
    for (uint32_t d : deltas) {
      clean();
      if (d % kP == 0) continue;
      st[i] =(uint32_t)(((uint64_t)st[i] + d % kP) % kP);
      const uint32_t want = rows < 2 ? unl : k + i;
      check("row", code, x, st, max_rows, true, &want);
    }
  // an input's alias x + p (x < 5) is no error
  {
    x[0] = 3;
    clean();
    std::vector<uint32_t> y = x;
    y[0] = 3 + kP;
    check("alias", code, y, st, max_rows, true, &locate::kNoSlot);
  }
  // random syndromes and double errors: rule == statement
  for (int n = 0; n < 20000; ++n) {
    clean();
    const int kind = n % 3;
    std::vector<uint32_t> y = x;
    if (kind == 0) {
      for (uint32_t i = 0; i < rows; ++i)
        if (rng() & 1) st[i] = (uint32_t)rng();
    } else if (kind == 1) {
      y[rng() % k] = word();
      st[rng() % rows] = (uint32_t)rng();
    } else {
      y[rng() % k] = word();
      y[rng() % k] = word();
    }
    check("random", code, y, st, max_rows, n < 12);
  }
}

}  // namespace

int main(int argc, char** argv) {
  print_cases = argc > 1 && strcmp(argv[1], "--cases") == 0;
  const int codes[][2] = {{3, 5}, {4, 6}, {8, 12}};
  uint64_t seed = 1;
  for (auto& c : codes)
    for (int rows = 1; rows <= c[1] - c[0]; ++rows) {
      const Code code = parity_code(c[0], c[1], rows);
      for (uint32_t mr = rows < 2 ? 2 : rows; mr <= (uint32_t)rows + 3; ++mr) run(code, mr, seed++);
    }
  // max_rows == rows == 1 is refused by the entry point, but the function is total: unlocated at k + 1
  run(parity_code(3, 5, 1), 1, seed++);
  if (failures) {
    printf("planset_locate_rule_test: %d failures\n", failures);
    return 1;
  }
  if (!print_cases) printf("planset_locate_rule_test ok (%llu columns)\n", (unsigned long long)checked);
  return 0;
}
