// The locate rule (slime_amd/csrc/locate_rule.hpp) on the CPU, over the product's
// parity matrices (rs_matrix.cpp) of 3/5, 4/6, 8/12, 10/14, 17/20, 33/50, 61/63 and
// 3/63 (the last two use all 63 slots: k = 61 with 2 rows, k = 3 with 60) and a
// matrix with zero entries:
//   every single-shard error in every slot, delta in {1, 4, p-1, 2^31}, random
//   deltas, and stored parity t + p for t < 5, is named;
//   a data symbol replaced by its alias x + p (x < 5) classifies clean;
//   10^5 random syndrome vectors and double errors per matrix agree with an
//   independent brute-force restatement (delta from s_0 c[0][j]^-1, then every
//   row compared).
//   locate_rule_test --cases prints planted cases for tests/locate_ref.py to be
//   pinned against: "rows k | coefficients | inputs | stored | slot" per line.
#include <stdint.h>
#include <stdio.h>
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

Code parity_code(int need, int total) {
  Matrix m;
  if (parity_matrix(need, total - need, &m) != Status::Ok) {
    printf("parity_matrix(%d, %d) failed\n", need, total - need);
    exit(1);
  }
  Code code{(uint32_t)need, (uint32_t)(total - need), {}};
  for (int i = need; i < total; ++i) code.c.insert(code.c.end(), m.row(i), m.row(i) + need);
  return code;
}

// Independent arithmetic: 128-bit sums, % p.
uint32_t dot(const Code& code, uint32_t i, const std::vector<uint32_t>& x) {
  u128 s = 0;
  for (uint32_t j = 0; j < code.k; ++j) s += (u128)code.row(i)[j] * x[j];
  return (uint32_t)(s % kP);
}

// The rule as the device runs it: rows fed one at a time.
uint32_t rule(const Code& code, const std::vector<uint32_t>& x, const std::vector<uint32_t>& stored) {
  locate::Column col;
  col.begin(code.k);
  for (uint32_t i = 0; i < code.rows; ++i) col.row(i, dot(code, i, x), stored[i], code.row(0), code.row(i));
  return col.slot(code.k, code.rows);
}

// The brute-force restatement: per-row flags and syndromes in arrays, delta by an inverse.
uint32_t brute(const Code& code, const std::vector<uint32_t>& x, const std::vector<uint32_t>& stored) {
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
  if (nd == 1) return code.k + last;
  uint32_t found = 0, which = 0;
  if (s[0] != 0) {
    for (uint32_t j = 0; j < code.k; ++j) {
      bool ok = true;
      if (code.row(0)[j] % kP == 0) {
        // s_i * 0 == s_0 * c[i][j] with s_0 != 0: every c[i][j] must be zero
        for (uint32_t i = 0; i < code.rows; ++i) ok = ok && code.row(i)[j] % kP == 0;
      } else {
        const uint64_t delta = s[0] * gf_minverse(code.row(0)[j] % kP) % kP;
        for (uint32_t i = 0; i < code.rows; ++i) ok = ok && s[i] == delta * (code.row(i)[j] % kP) % kP;
      }
      if (ok) {
        ++found;
        which = j;
      }
    }
  }
  return found == 1 ? which : code.k + code.rows;
}

int failures = 0;
bool print_cases = false;

void emit(const Code& code, const std::vector<uint32_t>& x, const std::vector<uint32_t>& stored, uint32_t slot) {
  if (!print_cases) return;
  printf("%u %u |", code.rows, code.k);
  for (uint32_t v : code.c) printf(" %u", v);
  printf(" |");
  for (uint32_t v : x) printf(" %u", v);
  printf(" |");
  for (uint32_t v : stored) printf(" %u", v);
  printf(" | %u\n", slot);
}

void expect(const char* what, const Code& code, const std::vector<uint32_t>& x, const std::vector<uint32_t>& stored,
            uint32_t want, bool keep = false) {
  const uint32_t got = rule(code, x, stored), ref = brute(code, x, stored);
  if (got != want || ref != want) {
    if (++failures <= 10) printf("FAIL %s (%u/%u): rule %u, brute force %u, planted %u\n", what, code.k, code.rows, got, ref, want);
  }
  if (keep) emit(code, x, stored, got);
}

void run(const Code& code, uint64_t seed, bool mds) {
  std::mt19937_64 rng(seed);
  auto word = [&]() { return (uint32_t)(rng() % kP); };
  const uint32_t k = code.k, rows = code.rows;
  std::vector<uint32_t> x(k), st(rows);
  for (uint32_t& v : x) v = word();
  for (uint32_t i = 0; i < rows; ++i) st[i] = dot(code, i, x);
  expect("clean", code, x, st, locate::kNoSlot, true);
  // every single-shard error in every slot
  std::vector<uint32_t> deltas = {1u, 4u, kP - 1, 1u << 31};
  for (int q = 0; q < 4; ++q) deltas.push_back(1 + (uint32_t)(rng() % (kP - 1)));
  for (uint32_t slot = 0; slot < k + rows; ++slot)
    for (size_t q = 0; q < deltas.size(); ++q) {
      const uint32_t dl = deltas[q];
      std::vector<uint32_t> xe = x, se = st;
      uint32_t want = slot;
      if (slot < k) {
        xe[slot] = (uint32_t)(((uint64_t)x[slot] + dl) % kP);
        // A matrix with zeros: an input that reaches one row only is, by the rule, that row; one
        // that reaches none is clean.  The MDS matrices have no zero entry.
        uint32_t hit = 0, lasthit = 0;
        for (uint32_t i = 0; i < rows; ++i)
          if (code.row(i)[slot] % kP) {
            ++hit;
            lasthit = i;
          }
        if (mds && hit != rows) {
          printf("FAIL: a zero in an MDS matrix\n");
          ++failures;
        }
        if (hit == 0) want = locate::kNoSlot;
        if (hit == 1) want = k + lasthit;
        if (!mds && hit >= 2) want = brute(code, xe, se);  // other columns may be proportional
      } else {
        se[slot - k] = (uint32_t)(((uint64_t)st[slot - k] + dl) % kP);
      }
      expect("single error", code, xe, se, want, q < 2 || q == 4);
    }
  // stored parity t + p for t < 5: bit-different, syndrome zero
  for (uint32_t t = 0; t < 5; ++t)
    for (uint32_t i = 0; i < rows; ++i) {
      // inputs that make row i compute t: solve through input j with c[i][j] != 0
      std::vector<uint32_t> xe = x;
      uint32_t j = 0;
      while (j < k && code.row(i)[j] % kP == 0) ++j;
      if (j == k) continue;
      const uint32_t comp = dot(code, i, xe);
      const uint64_t need = ((uint64_t)t + kP - comp) % kP;  // add need to row i through input j
      xe[j] = (uint32_t)((xe[j] + need * gf_minverse(code.row(i)[j] % kP) % kP) % kP);
      std::vector<uint32_t> se(rows);
      for (uint32_t r = 0; r < rows; ++r) se[r] = dot(code, r, xe);
      if (se[i] != t) {
        printf("FAIL: could not steer row %u to %u\n", i, t);
        ++failures;
        continue;
      }
      se[i] = t + kP;  // fits: t < 5
      expect("stored alias", code, xe, se, k + i, true);
    }
  // a data symbol replaced by its alias x + p classifies clean
  for (uint32_t t = 0; t < 5; ++t)
    for (uint32_t j = 0; j < k; ++j) {
      std::vector<uint32_t> xe = x, se(rows);
      xe[j] = t;
      for (uint32_t r = 0; r < rows; ++r) se[r] = dot(code, r, xe);
      xe[j] = t + kP;
      expect("input alias", code, xe, se, locate::kNoSlot, j == 0);
    }
  // random syndromes and double errors against the brute force
  for (int n = 0; n < 100000; ++n) {
    std::vector<uint32_t> xe = x, se = st;
    const int kind = n % 4;
    if (kind == 0) {
      for (uint32_t& v : se) v = (uint32_t)rng();  // any uint32, aliases included
    } else if (kind == 1) {
      for (uint32_t& v : se) v = (rng() & 3) ? v : word();
    } else {  // two wrong shards in one column
      const uint32_t a = (uint32_t)(rng() % (k + rows));
      uint32_t b = (uint32_t)(rng() % (k + rows - 1));
      if (b >= a) ++b;
      for (uint32_t sl : {a, b}) {
        if (sl < k)
          xe[sl] = kind == 2 ? word() : (uint32_t)rng();
        else
          se[sl - k] = kind == 2 ? word() : (uint32_t)rng();
      }
    }
    const uint32_t got = rule(code, xe, se), ref = brute(code, xe, se);
    if (got != ref && ++failures <= 10) printf("FAIL random %d (%u/%u): rule %u, brute force %u\n", n, k, rows, got, ref);
    if (n < 24) emit(code, xe, se, got);
  }
}

}  // namespace

int main(int argc, char** argv) {
  print_cases = argc > 1 && !strcmp(argv[1], "--cases");
  // 61/63 and 3/63 fill all 63 slots: `cand` starts with bits above 32 set, and 60 rows feed it.
  const int codes[][2] = {{3, 5}, {4, 6}, {8, 12}, {10, 14}, {17, 20}, {33, 50}, {61, 63}, {3, 63}};
  for (const auto& c : codes) run(parity_code(c[0], c[1]), 1000 * c[0] + c[1], true);
  // A matrix with zero entries: a zero in row 0, a zero below it, an input that reaches one row
  // only, one that reaches none, and two proportional columns.
  Code z{6, 3, {0, 5, 7, 0, 2, 4,  //
                3, 0, 9, 0, 3, 6,  //
                1, 2, 0, 0, 0, 0}};
  run(z, 77, false);
  if (failures) {
    printf("locate_rule_test: %d failures\n", failures);
    return 1;
  }
  printf("locate_rule_test ok\n");
  return 0;
}
