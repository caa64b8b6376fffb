// The pair rule (slime_amd/csrc/locate_rule.hpp, pair_slots) on the CPU, over the
// product's parity matrices (rs_matrix.cpp) of 3/7, 4/8, 8/12, 10/14, 16/20, 17/21,
// 3/12 (nine rows), 33/50, 59/63 and 3/63 (the last two use all 63 slots) and over
// matrices with zero entries and dependent columns, against an independent
// brute-force statement: ranks and coefficients by Gaussian elimination with
// inverses, every pair counted, nothing cross-multiplied.
//   every pair of slots planted, deltas from the edge values and random ones,
//     must be named (MDS matrices) -- or be what the brute force says (the others);
//   stored rows that are non-canonical aliases: bit-different, syndrome zero;
//   every single error must still give the one-shard rule's slot;
//   planted triples are unlocated;
//   10^5 random syndromes per matrix agree with the brute force;
//   a plan of three rows answers as the one-shard rule does;
//   at 59/63 and 3/63 every one of the 63 slots and `unlocated` are named.
// locate_pairs_rule_test --cases prints planted cases for tests/locate_pairs_ref.py
// to be pinned against: "rows k | coefficients | inputs | stored | a b" per line,
// b = 4294967295 unless the column is a pair.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <set>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
#include "locate_rule.hpp"
#include "rs_matrix.hpp"

using namespace slime;

namespace {

typedef unsigned __int128 u128;
typedef std::vector<uint32_t> Words;

struct Code {
  uint32_t k, rows;
  Words c;  // rows x k
  const uint32_t* row(uint32_t i) const { return c.data() + (size_t)i * k; }
  uint32_t slots() const { return k + rows; }
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
uint32_t dot(const Code& code, uint32_t i, const Words& x) {
  u128 s = 0;
  for (uint32_t j = 0; j < code.k; ++j) s += (u128)code.row(i)[j] * x[j];
  return (uint32_t)(s % kP);
}
uint64_t mulm(uint64_t a, uint64_t b) { return a * b % kP; }  // a, b < 2^32
uint64_t subm(uint64_t a, uint64_t b) { return (a + kP - b) % kP; }

struct Answer {
  uint32_t a, b;
  bool operator==(const Answer& o) const { return a == o.a && b == o.b; }
  bool operator!=(const Answer& o) const { return !(*this == o); }
};

// The rule as the device runs it: rows fed one at a time, the syndromes kept in an array that the
// rule reads through an accessor, the d_i in a mask.
Answer rule(const Code& code, const Words& x, const Words& stored) {
  locate::Column col;
  col.begin(code.k);
  Words syn(code.rows);
  uint64_t dmask = 0;
  for (uint32_t i = 0; i < code.rows; ++i) {
    const uint32_t comp = dot(code, i, x);
    col.row(i, comp, stored[i], code.row(0), code.row(i));
    dmask |= (uint64_t)(stored[i] != comp) << i;
    syn[i] = locate::sub(canon(stored[i]), comp);
  }
  const locate::Slots r = locate::pair_slots(
      col.slot(code.k, code.rows), dmask, [&](uint32_t i) { return syn[i]; },
      [&](uint32_t i, uint32_t j) { return code.row(i)[j]; }, code.k, code.rows);
  return Answer{r.a, r.b};
}

// h_a[i] mod p.
uint64_t hcol(const Code& code, uint32_t a, uint32_t i) {
  return a < code.k ? code.row(i)[a] % kP : (a - code.k == i ? 1u : 0u);
}

// What the elimination of [h_a h_b] needs, which does not depend on the syndrome: the pivot rows
// and the pivots' inverses.  independent == false: rank below two.
struct Elim {
  bool independent;
  uint32_t r1, r2;
  uint64_t inv1, inv2;  // 1 / h_a[r1], 1 / (h_b[r2] - h_b[r1] h_a[r2] / h_a[r1])
};

struct Brute {
  const Code& code;
  std::vector<Elim> elim;  // a * slots + b, a < b
  explicit Brute(const Code& c) : code(c), elim((size_t)c.slots() * c.slots()) {
    const uint32_t n = code.slots(), rows = code.rows;
    for (uint32_t a = 0; a < n; ++a)
      for (uint32_t b = a + 1; b < n; ++b) {
        Elim e{false, 0, 0, 0, 0};
        uint32_t r1 = 0;
        while (r1 < rows && hcol(code, a, r1) == 0) ++r1;
        if (r1 < rows) {
          e.r1 = r1;
          e.inv1 = gf_minverse((uint32_t)hcol(code, a, r1));
          const uint64_t f = mulm(hcol(code, b, r1), e.inv1);  // h_b' = h_b - f h_a
          for (uint32_t r2 = 0; r2 < rows; ++r2) {
            if (r2 == r1) continue;
            const uint64_t v = subm(hcol(code, b, r2), mulm(f, hcol(code, a, r2)));
            if (v != 0) {
              e.independent = true;
              e.r2 = r2;
              e.inv2 = gf_minverse((uint32_t)v);
              break;
            }
          }
        }
        elim[(size_t)a * n + b] = e;
      }
  }
  // s = alpha h_a + beta h_b with alpha, beta != 0: solve by the two pivots, compare every row.
  bool explains(const std::vector<uint64_t>& s, uint32_t a, uint32_t b) const {
    const Elim& e = elim[(size_t)a * code.slots() + b];
    if (!e.independent) return false;
    const uint64_t f = mulm(hcol(code, b, e.r1), e.inv1);
    const uint64_t g = mulm(s[e.r1], e.inv1);  // s' = s - g h_a
    const uint64_t beta = mulm(subm(s[e.r2], mulm(g, hcol(code, a, e.r2))), e.inv2);
    const uint64_t alpha = subm(g, mulm(beta, f));
    if (alpha == 0 || beta == 0) return false;
    for (uint32_t i = 0; i < code.rows; ++i)
      if (s[i] != (mulm(alpha, hcol(code, a, i)) + mulm(beta, hcol(code, b, i))) % kP) return false;
    return true;
  }
  Answer operator()(const Words& x, const Words& stored) const {
    const uint32_t k = code.k, rows = code.rows, un = k + rows;
    std::vector<uint64_t> s(rows);
    std::vector<uint32_t> d;
    for (uint32_t i = 0; i < rows; ++i) {
      const uint32_t comp = dot(code, i, x);
      if (stored[i] != comp) d.push_back(i);
      s[i] = subm(stored[i] % kP, comp);
    }
    if (d.empty()) return Answer{locate::kNoSlot, locate::kNoSlot};
    if (d.size() == 1) return Answer{k + d[0], locate::kNoSlot};
    // one input: delta from s_0 / c[0][j], every row compared
    uint32_t found = 0, which = 0;
    if (s[0] != 0)
      for (uint32_t j = 0; j < k; ++j) {
        bool ok = true;
        if (hcol(code, j, 0) == 0) {
          for (uint32_t i = 0; i < rows; ++i) ok = ok && hcol(code, j, i) == 0;
        } else {
          const uint64_t delta = mulm(s[0], gf_minverse((uint32_t)hcol(code, j, 0)));
          for (uint32_t i = 0; i < rows && ok; ++i) ok = s[i] == mulm(delta, hcol(code, j, i));
        }
        if (ok) {
          ++found;
          which = j;
        }
      }
    if (found == 1) return Answer{which, locate::kNoSlot};
    if (rows < 4) return Answer{un, locate::kNoSlot};
    if (d.size() == 2) return Answer{k + d[0], k + d[1]};
    uint32_t np = 0;
    Answer pair{un, locate::kNoSlot};
    for (uint32_t a = 0; a < un; ++a)
      for (uint32_t b = a + 1; b < un; ++b)
        if (explains(s, a, b)) {
          ++np;
          pair = Answer{a, b};
        }
    return np == 1 ? pair : Answer{un, locate::kNoSlot};
  }
};

int failures = 0;
bool print_cases = false;

void emit(const Code& code, const Words& x, const Words& stored, Answer r) {
  if (!print_cases) return;
  printf("%u %u |", code.rows, code.k);
  for (uint32_t v : code.c) printf(" %u", v);
  printf(" |");
  for (uint32_t v : x) printf(" %u", v);
  printf(" |");
  for (uint32_t v : stored) printf(" %u", v);
  printf(" | %u %u\n", r.a, r.b);
}

struct Seen {
  std::set<uint32_t> slots;
  void note(Answer r) {
    slots.insert(r.a);
    if (r.b != locate::kNoSlot) slots.insert(r.b);
  }
};

// got must equal the brute force; `want` too unless null.
Answer expect(const char* what, const Code& code, const Brute& brute, const Words& x, const Words& stored,
              const Answer* want, bool keep, Seen* seen = nullptr) {
  const Answer got = rule(code, x, stored), ref = brute(x, stored);
  if (got != ref || (want && got != *want)) {
    if (++failures <= 10)
      printf("FAIL %s (%u/%u): rule %u %u, brute force %u %u, planted %u %u\n", what, code.k, code.rows, got.a, got.b,
             ref.a, ref.b, want ? want->a : 0, want ? want->b : 0);
  }
  if (keep) {
    emit(code, x, stored, got);
    if (seen) seen->note(got);
  }
  return got;
}

// Adds delta (mod p) to slot sl of the column (x, st); alias: the stored row is replaced by its
// non-canonical alias instead where it has one (computed < 5), which leaves the syndrome alone.
void damage(const Code& code, Words& x, Words& st, uint32_t sl, uint32_t delta) {
  if (sl < code.k)
    x[sl] = (uint32_t)(((uint64_t)x[sl] % kP + delta) % kP);
  else
    st[sl - code.k] = (uint32_t)(((uint64_t)st[sl - code.k] % kP + delta) % kP);
}

void run(const Code& code, uint64_t seed, bool mds, bool all_slots) {
  std::mt19937_64 rng(seed);
  auto word = [&]() { return (uint32_t)(rng() % kP); };
  const uint32_t k = code.k, rows = code.rows, n = k + rows;
  const Brute brute(code);
  Seen seen;
  Words x(k), st(rows);
  for (uint32_t& v : x) v = word();
  for (uint32_t i = 0; i < rows; ++i) st[i] = dot(code, i, x);
  const Answer clean{locate::kNoSlot, locate::kNoSlot}, unlocated{n, locate::kNoSlot};
  expect("clean", code, brute, x, st, &clean, true);

  // every single error still gives the one-shard rule's slot
  const uint32_t edges[] = {1u, 4u, kP - 1, 1u << 31};
  for (uint32_t sl = 0; sl < n; ++sl)
    for (int q = 0; q < 6; ++q) {
      Words xe = x, se = st;
      damage(code, xe, se, sl, q < 4 ? edges[q] : 1 + (uint32_t)(rng() % (kP - 1)));
      const Answer one{sl, locate::kNoSlot};
      expect("single error", code, brute, xe, se, mds ? &one : nullptr, q == 0 || q == 5, &seen);
    }

  // every pair of slots, deltas from the edge values and random ones
  uint32_t turn = 0;
  for (uint32_t a = 0; a < n; ++a)
    for (uint32_t b = a + 1; b < n; ++b, ++turn) {
      for (int q = 0; q < 3; ++q) {
        Words xe = x, se = st;
        const uint32_t da = q == 0 ? edges[turn % 4] : 1 + (uint32_t)(rng() % (kP - 1));
        const uint32_t db = q == 1 ? edges[(turn / 4) % 4] : 1 + (uint32_t)(rng() % (kP - 1));
        damage(code, xe, se, a, da);
        damage(code, xe, se, b, db);
        const Answer both{a, b};
        // kept: the pairs of neighbouring slots and of slots half the code apart -- every slot is a
        // member -- and every 97th
        const bool keep = q == 0 && (b == a + 1 || b == a + n / 2 || turn % 97 == 0);
        if (print_cases && !keep) continue;  // --cases prints the kept ones only
        expect("planted pair", code, brute, xe, se, mds && rows >= 4 ? &both : nullptr, keep, &seen);
      }
    }

  // stored rows that are non-canonical aliases: inputs steered so that rows i1 (and i2) compute
  // t < 5, then stored as t + p.  Two aliased rows are case 3 with a zero syndrome; an aliased row
  // beside a wrong input is the input alone (the alias is invisible to the syndrome and the
  // one-shard rule answers first); an aliased row beside a wrong row is case 3.
  if (mds && rows >= 4 && k >= 2) {
    for (uint32_t t = 0; t < 5; ++t)
      for (uint32_t i1 = 0; i1 < rows; ++i1) {
        const uint32_t i2 = (i1 + 1 + t) % rows;
        if (i2 == i1) continue;
        // two equations in inputs 0 and 1: row i1 -> t, row i2 -> t + 1 (mod 5)
        Words xe = x;
        const uint64_t a11 = hcol(code, 0, i1), a12 = hcol(code, 1, i1), a21 = hcol(code, 0, i2), a22 = hcol(code, 1, i2);
        const uint64_t det = subm(mulm(a11, a22), mulm(a12, a21));
        if (det == 0) continue;
        const uint32_t t2 = (t + 1) % 5;
        const uint64_t n1 = subm(t, dot(code, i1, xe)), n2 = subm(t2, dot(code, i2, xe));
        const uint64_t inv = gf_minverse((uint32_t)det);
        const uint64_t u = mulm(subm(mulm(n1, a22), mulm(n2, a12)), inv), v = mulm(subm(mulm(a11, n2), mulm(a21, n1)), inv);
        xe[0] = (uint32_t)((xe[0] + u) % kP);
        xe[1] = (uint32_t)((xe[1] + v) % kP);
        Words se(rows);
        for (uint32_t r = 0; r < rows; ++r) se[r] = dot(code, r, xe);
        if (se[i1] != t || se[i2] != t2) {
          printf("FAIL: could not steer rows %u, %u\n", i1, i2);
          ++failures;
          continue;
        }
        Words two = se;
        two[i1] = t + kP;
        two[i2] = t2 + kP;
        const Answer rows2{k + (i1 < i2 ? i1 : i2), k + (i1 < i2 ? i2 : i1)};
        expect("two aliased rows", code, brute, xe, two, &rows2, true, &seen);
        Words mixed = se;  // one alias, one wrong value
        mixed[i1] = t + kP;
        mixed[i2] = (uint32_t)((t2 + 1 + rng() % (kP - 1)) % kP);
        expect("aliased row and wrong row", code, brute, xe, mixed, &rows2, t == 0);
        Words xa = xe, sa = se;  // one alias beside a wrong input: the input alone
        const uint32_t j = (uint32_t)(rng() % k);
        xa[j] = (uint32_t)((xa[j] + 1 + rng() % (kP - 1)) % kP);
        sa[i1] = t + kP;
        const Answer input{j, locate::kNoSlot};
        expect("aliased row and wrong input", code, brute, xa, sa, &input, t == 0);
      }
  }

  // planted triples: unlocated (a wrong pair is blamed with probability about n^2 / (2 p^(rows-2)))
  for (int t = 0; t < 300; ++t) {
    uint32_t sl[3];
    sl[0] = (uint32_t)(rng() % n);
    do sl[1] = (uint32_t)(rng() % n); while (sl[1] == sl[0]);
    do sl[2] = (uint32_t)(rng() % n); while (sl[2] == sl[0] || sl[2] == sl[1]);
    Words xe = x, se = st;
    for (uint32_t v : sl) damage(code, xe, se, v, 1 + (uint32_t)(rng() % (kP - 1)));
    expect("planted triple", code, brute, xe, se, mds ? &unlocated : nullptr, t < 6, &seen);
  }

  // random syndromes against the brute force
  for (int t = 0; t < (print_cases ? 24 : 100000); ++t) {
    Words xe = x, se = st;
    const int kind = t % 4;
    if (kind == 0) {
      for (uint32_t& v : se) v = (uint32_t)rng();  // any uint32, aliases included
    } else if (kind == 1) {
      for (uint32_t& v : se) v = (rng() & 3) ? v : word();  // a few rows wrong
    } else if (kind == 2) {  // a combination of two columns, zero coefficients included
      const uint32_t a = (uint32_t)(rng() % n), b = (uint32_t)(rng() % n);
      const uint32_t al = (rng() & 7) ? word() : 0, be = (rng() & 7) ? word() : 0;
      for (uint32_t i = 0; i < rows; ++i)
        se[i] = (uint32_t)((st[i] + mulm(al, hcol(code, a, i)) + mulm(be, hcol(code, b, i))) % kP);
    } else {  // two or three wrong slots, any uint32
      const int m = 2 + (int)(rng() & 1);
      for (int q = 0; q < m; ++q) {
        const uint32_t sl = (uint32_t)(rng() % n);
        if (sl < k)
          xe[sl] = (uint32_t)rng();
        else
          se[sl - k] = (uint32_t)rng();
      }
    }
    const Answer got = rule(code, xe, se), ref = brute(xe, se);
    if (got != ref && ++failures <= 10)
      printf("FAIL random %d (%u/%u): rule %u %u, brute force %u %u\n", t, k, rows, got.a, got.b, ref.a, ref.b);
    if (t < 24) {
      emit(code, xe, se, got);
      seen.note(got);
    }
  }
  if (all_slots)
    for (uint32_t sl = 0; sl <= n; ++sl)
      if (!seen.slots.count(sl)) {
        printf("FAIL (%u/%u): slot %u is never named in the kept cases\n", k, rows, sl);
        ++failures;
      }
}

}  // namespace

int main(int argc, char** argv) {
  print_cases = argc > 1 && !strcmp(argv[1], "--cases");
  const int codes[][2] = {{3, 7}, {4, 8}, {8, 12}, {10, 14}, {16, 20}, {17, 21}, {3, 12}, {33, 50}, {59, 63}, {3, 63}};
  for (const auto& c : codes) run(parity_code(c[0], c[1]), 1000 * c[0] + c[1], true, c[1] == 63);
  // Three rows: the pair rule answers as the one-shard rule does.
  run(parity_code(5, 8), 5008, true, false);
  // Matrices with zeros and dependent columns: inputs that reach one row, two rows or none,
  // proportional columns, a column equal to a unit vector, a column that is the sum of two others.
  Code z{6, 4, {0, 5, 7, 0, 2, 4,  //
                3, 0, 9, 0, 3, 6,  //
                1, 2, 0, 0, 0, 0,  //
                0, 0, 4, 0, 5, 10}};
  run(z, 77, false, false);
  Code y{5, 5, {1, 2, 3, 0, 3,  //
                1, 3, 4, 0, 5,  //
                1, 4, 5, 1, 7,  //
                1, 5, 6, 0, 9,  //
                1, 6, 7, 0, 11}};
  run(y, 78, false, false);
  if (failures) {
    printf("locate_pairs_rule_test: %d failures\n", failures);
    return 1;
  }
  printf("locate_pairs_rule_test ok\n");
  return 0;
}
