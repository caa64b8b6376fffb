// The correct rule (slime_amd/csrc/correct_rule.hpp) on the CPU, behind both locate
// rules of locate_rule.hpp, over the product's parity matrices (rs_matrix.cpp) of
// 3/7, 4/8, 8/12, 10/14, 16/20, 17/21, 3/12, 33/50, 59/63 and 3/63 and over the two
// degenerate matrices of locate_pairs_rule_test (zero and proportional columns, a
// unit-vector column).  The column is corrected the way the device does it: classify,
// take the Fix, form every new word from the column as stored, then store.
//   inv: a inv(a) == 1 at the edge values and 10^5 random ones;
//   every single slot planted, edge and random deltas: the column comes back exactly;
//   every pair of slots planted (input+input, input+row, row+row): likewise;
//   non-canonical words p + t: a damaged word whose original was an alias comes back
//     as its residue, an aliased stored row is rewritten canonical, an aliased
//     bystander input is left bit for bit;
//   degenerate matrices: the outcome is the locate rule's slots and a clean column, or
//     "unsolvable -> unlocated" with nothing written, which happens only for a named
//     input whose coefficient column is all zero -- never a write that leaves the
//     column dirty.  The slots are compared with locate_rule.hpp's own answer, not with
//     a brute force: locate_pairs_rule_test brute-forces the slots on these matrices;
//     what this program adds, and what carries the weight here, is the independent
//     check (128-bit dot products) that every written column verifies clean.
// correct_rule_test --cases prints planted cases for tests/correct_ref.py to be pinned
// against: "rows k | coefficients | inputs | stored | max_wrong | a b | inputs after |
// stored after" per line, b = 4294967295 unless the column is a pair.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
#include "correct_rule.hpp"
#include "rs_matrix.hpp"

using namespace slime;

namespace {

typedef unsigned __int128 u128;
typedef std::vector<uint32_t> Words;

struct Code {
  uint32_t k, rows;
  Words c;  // rows x k
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
uint32_t dot(const Code& code, uint32_t i, const Words& x) {
  u128 s = 0;
  for (uint32_t j = 0; j < code.k; ++j) s += (u128)code.row(i)[j] * x[j];
  return (uint32_t)(s % kP);
}

int failures = 0;
bool print_cases = false;

void fail(const char* what, const Code& code, uint32_t a, uint32_t b) {
  if (++failures <= 10) printf("FAIL %s (%u/%u) slots %u %u\n", what, code.k, code.rows, a, b);
}

struct Outcome {
  uint32_t a, b;  // the slots to tally
  bool wrote;
};

// One column through the rule and the fix, as correct_column (rs_correct_ragged.hip) does it.
Outcome correct(const Code& code, Words& x, Words& st, int max_wrong) {
  const uint32_t k = code.k, rows = code.rows;
  locate::Column col;
  col.begin(k);
  Words syn(rows);
  uint64_t dmask = 0;
  for (uint32_t i = 0; i < rows; ++i) {
    const uint32_t comp = dot(code, i, x);
    col.row(i, comp, st[i], code.row(0), code.row(i));
    dmask |= (uint64_t)(st[i] != comp) << i;
    syn[i] = locate::sub(canon(st[i]), comp);
  }
  auto s = [&](uint32_t i) { return syn[i]; };
  auto c = [&](uint32_t i, uint32_t j) { return code.row(i)[j]; };
  locate::Slots ps{col.slot(k, rows), locate::kNoSlot};
  if (max_wrong == 2) ps = locate::pair_slots(ps.a, dmask, s, c, k, rows);
  if (ps.a == locate::kNoSlot || ps.a == k + rows) return Outcome{ps.a, ps.b, false};
  const correct::Fix f = ps.b == locate::kNoSlot ? correct::single_fix(s, c, k, rows, ps.a)
                                                 : correct::pair_fix(s, c, k, rows, ps.a, ps.b);
  if (!f.solved) return Outcome{k + rows, locate::kNoSlot, false};
  auto value = [&](uint32_t slot, uint32_t d) {
    return locate::add(slot < k ? canon(x[slot]) : dot(code, slot - k, x), d);
  };
  auto put = [&](uint32_t slot, uint32_t v) { (slot < k ? x[slot] : st[slot - k]) = v; };
  const uint32_t va = value(ps.a, f.da);
  if (ps.b != locate::kNoSlot) put(ps.b, value(ps.b, f.db));
  put(ps.a, va);
  return Outcome{ps.a, ps.b, true};
}

void emit(const Code& code, const Words& x, const Words& st, int max_wrong, Outcome o, const Words& xa,
          const Words& sa) {
  if (!print_cases) return;
  printf("%u %u |", code.rows, code.k);
  for (uint32_t v : code.c) printf(" %u", v);
  printf(" |");
  for (uint32_t v : x) printf(" %u", v);
  printf(" |");
  for (uint32_t v : st) printf(" %u", v);
  printf(" | %d | %u %u |", max_wrong, o.a, o.b);
  for (uint32_t v : xa) printf(" %u", v);
  printf(" |");
  for (uint32_t v : sa) printf(" %u", v);
  printf("\n");
}

bool column_clean(const Code& code, const Words& x, const Words& st) {
  for (uint32_t i = 0; i < code.rows; ++i)
    if (st[i] != dot(code, i, x)) return false;
  return true;
}

void damage(const Code& code, Words& x, Words& st, uint32_t sl, uint32_t delta) {
  uint32_t& w = sl < code.k ? x[sl] : st[sl - code.k];
  w = (uint32_t)(((uint64_t)w % kP + delta) % kP);
}

// Corrects (xe, se) and expects slots {a, b} and the column (x, st) back.
void expect_restored(const char* what, const Code& code, const Words& x, const Words& st, Words xe, Words se,
                     int max_wrong, uint32_t a, uint32_t b, bool keep) {
  const Words x0 = xe, s0 = se;
  const Outcome o = correct(code, xe, se, max_wrong);
  if (o.a != a || o.b != b || !o.wrote || xe != x || se != st) fail(what, code, a, b);
  if (keep) emit(code, x0, s0, max_wrong, o, xe, se);
}

void run_mds(const Code& code, uint64_t seed) {
  std::mt19937_64 rng(seed);
  auto word = [&]() { return (uint32_t)(rng() % kP); };
  const uint32_t k = code.k, rows = code.rows, n = k + rows;
  Words x(k), st(rows);
  for (uint32_t& v : x) v = word();
  for (uint32_t i = 0; i < rows; ++i) st[i] = dot(code, i, x);
  for (int mw = 1; mw <= 2; ++mw) {  // a clean column: nothing named, nothing written
    Words xe = x, se = st;
    const Outcome o = correct(code, xe, se, mw);
    if (o.a != locate::kNoSlot || o.wrote || xe != x || se != st) fail("clean", code, o.a, o.b);
    emit(code, x, st, mw, o, xe, se);
  }

  const uint32_t edges[] = {1u, 2u, kP - 1, kP - 2, 1u << 31, (1u << 31) + 1, (1u << 31) - 1};
  for (uint32_t sl = 0; sl < n; ++sl)
    for (int q = 0; q < 10; ++q) {
      Words xe = x, se = st;
      damage(code, xe, se, sl, q < 7 ? edges[q] : 1 + (uint32_t)(rng() % (kP - 1)));
      for (int mw = 1; mw <= 2; ++mw)
        expect_restored("single slot", code, x, st, xe, se, mw, sl, locate::kNoSlot, q == 2 || q == 9);
    }

  if (rows >= 4) {
    uint32_t turn = 0;
    for (uint32_t a = 0; a < n; ++a)
      for (uint32_t b = a + 1; b < n; ++b, ++turn) {
        const bool keep = b == a + 1 || b == a + n / 2 || turn % 97 == 0;
        if (print_cases && !keep) continue;
        for (int q = 0; q < 3; ++q) {
          Words xe = x, se = st;
          damage(code, xe, se, a, q == 0 ? edges[turn % 7] : 1 + (uint32_t)(rng() % (kP - 1)));
          damage(code, xe, se, b, q == 1 ? edges[(turn / 7) % 7] : 1 + (uint32_t)(rng() % (kP - 1)));
          expect_restored("planted pair", code, x, st, xe, se, 2, a, b, keep && q == 0);
        }
      }
    // the one-shard rule leaves a pair alone
    Words xe = x, se = st;
    damage(code, xe, se, 0, 5);
    damage(code, xe, se, k, 7);
    const Words x0 = xe, s0 = se;
    const Outcome o = correct(code, xe, se, 1);
    if (o.a != n || o.wrote || xe != x0 || se != s0) fail("pair under the one-shard rule", code, o.a, o.b);
    emit(code, x0, s0, 1, o, xe, se);
  }

  // Non-canonical words.  Input 0 is steered so that row i computes t < 5; then
  //   the stored row as the alias t + p: row i named, rewritten as t;
  //   an original input 1 of value t, stored as t + p beside a wrong slot: left bit for bit
  //     (the corrected column is the aliased one);
  //   the same input damaged: it comes back as t, its residue.
  for (uint32_t t = 0; t < 5; ++t)
    for (uint32_t i = 0; i < rows; ++i) {
      Words xa = x;
      if (k >= 2) xa[1] = t;
      const uint32_t c0 = canon(code.row(i)[0]);
      xa[0] = locate::add(xa[0], locate::mul(locate::sub(t, dot(code, i, xa)), correct::inv(c0)));
      Words sa(rows);
      for (uint32_t r = 0; r < rows; ++r) sa[r] = dot(code, r, xa);
      if (sa[i] != t) {
        fail("could not steer", code, i, t);
        continue;
      }
      for (int mw = 1; mw <= 2; ++mw) {
        Words se = sa;
        se[i] = t + kP;
        expect_restored("aliased stored row", code, xa, sa, xa, se, mw, k + i, locate::kNoSlot, mw == 1);
        if (k < 2) continue;
        Words xal = xa;  // the column with input 1 stored as its alias
        xal[1] = t + kP;
        Words xe = xal;
        se = sa;
        damage(code, xe, se, k + i, 1 + (uint32_t)(rng() % (kP - 1)));
        expect_restored("aliased bystander", code, xal, sa, xe, se, mw, k + i, locate::kNoSlot, false);
        xe = xal;
        xe[1] = 1 + t + (uint32_t)(rng() % (kP - 6));  // != t mod p
        expect_restored("aliased original", code, xa, sa, xe, sa, mw, 1, locate::kNoSlot, mw == 2 && i == 0);
      }
    }
}

// Degenerate matrices: whatever the rule names, a write leaves the column clean; "unsolvable" only
// for a named input with an all-zero coefficient column, and then nothing is written.
void run_degenerate(const Code& code, uint64_t seed) {
  std::mt19937_64 rng(seed);
  auto word = [&]() { return (uint32_t)(rng() % kP); };
  const uint32_t k = code.k, rows = code.rows, n = k + rows;
  Words x(k), st(rows);
  for (uint32_t& v : x) v = word();
  for (uint32_t i = 0; i < rows; ++i) st[i] = dot(code, i, x);
  auto zero_column = [&](uint32_t j) {
    for (uint32_t i = 0; i < rows; ++i)
      if (canon(code.row(i)[j]) != 0) return false;
    return true;
  };
  int unsolvable = 0, wrote = 0;
  auto check = [&](const Words& xe, const Words& se, bool keep) {
    for (int mw = 1; mw <= 2; ++mw) {
      Words xc = xe, sc = se;
      // what locate alone says
      locate::Column col;
      col.begin(k);
      Words syn(rows);
      uint64_t dmask = 0;
      for (uint32_t i = 0; i < rows; ++i) {
        const uint32_t comp = dot(code, i, xe);
        col.row(i, comp, se[i], code.row(0), code.row(i));
        dmask |= (uint64_t)(se[i] != comp) << i;
        syn[i] = locate::sub(canon(se[i]), comp);
      }
      locate::Slots ps{col.slot(k, rows), locate::kNoSlot};
      if (mw == 2)
        ps = locate::pair_slots(
            ps.a, dmask, [&](uint32_t i) { return syn[i]; }, [&](uint32_t i, uint32_t j) { return code.row(i)[j]; }, k,
            rows);
      const Outcome o = correct(code, xc, sc, mw);
      if (o.wrote) {
        ++wrote;
        if (o.a != ps.a || o.b != ps.b || !column_clean(code, xc, sc)) fail("a write left the column dirty", code, o.a, o.b);
      } else {
        if (xc != xe || sc != se) fail("written without a fix", code, o.a, o.b);
        const bool named = ps.a != locate::kNoSlot && ps.a != n;
        if (named) {  // unsolvable -> unlocated
          ++unsolvable;
          if (o.a != n || o.b != locate::kNoSlot || ps.b != locate::kNoSlot || ps.a >= k || !zero_column(ps.a))
            fail("unsolvable", code, ps.a, ps.b);
        } else if (o.a != ps.a) {
          fail("outcome differs from locate", code, o.a, ps.a);
        }
      }
      if (keep) emit(code, xe, se, mw, o, xc, sc);
    }
  };
  for (uint32_t a = 0; a < n; ++a) {
    Words xe = x, se = st;
    damage(code, xe, se, a, 1 + (uint32_t)(rng() % (kP - 1)));
    check(xe, se, true);
    for (uint32_t b = a + 1; b < n; ++b)
      for (int q = 0; q < 3; ++q) {
        Words xp = xe, sp = se;
        damage(code, xp, sp, b, 1 + (uint32_t)(rng() % (kP - 1)));
        check(xp, sp, q == 0);
      }
  }
  for (int t = 0; t < (print_cases ? 24 : 100000); ++t) {
    Words xe = x, se = st;
    if (t % 2 == 0) {
      for (uint32_t& v : se) v = (rng() & 3) ? v : word();  // a few rows wrong
    } else {  // a combination of two columns, zero coefficients included
      const uint32_t a = (uint32_t)(rng() % n), b = (uint32_t)(rng() % n);
      const uint32_t al = (rng() & 7) ? word() : 0, be = (rng() & 7) ? word() : 0;
      auto h = [&](uint32_t sl, uint32_t i) { return sl < k ? code.row(i)[sl] % kP : (sl - k == i ? 1u : 0u); };
      for (uint32_t i = 0; i < rows; ++i)
        se[i] = (uint32_t)((st[i] + (uint64_t)al * h(a, i) % kP + (uint64_t)be * h(b, i) % kP) % kP);
    }
    check(xe, se, t < 24);
  }
  if (!print_cases && wrote == 0) fail("no write among the degenerate cases", code, 0, 0);
  if (!print_cases) printf("degenerate %u/%u: %d writes, %d unsolvable\n", k, rows, wrote, unsolvable);
}

void test_inv() {
  std::mt19937_64 rng(99);
  const uint32_t edges[] = {1u, 2u, kP - 1, kP - 2, (1u << 31) + 1, (1u << 31) - 1, 1u << 31};
  auto one = [&](uint32_t a) {
    const uint32_t r = correct::inv(a);
    if (r >= kP || (u128)a * r % kP != 1) {
      if (++failures <= 10) printf("FAIL inv(%u) = %u\n", a, r);
    }
  };
  for (uint32_t a : edges) one(a);
  for (int t = 0; t < 100000; ++t) one(1 + (uint32_t)(rng() % (kP - 1)));
  if (correct::inv(0) != 0) {
    printf("FAIL inv(0)\n");
    ++failures;
  }
}

}  // namespace

int main(int argc, char** argv) {
  print_cases = argc > 1 && !strcmp(argv[1], "--cases");
  test_inv();
  const int codes[][2] = {{3, 7}, {4, 8}, {8, 12}, {10, 14}, {16, 20}, {17, 21}, {3, 12}, {33, 50}, {59, 63}, {3, 63}};
  for (const auto& c : codes) run_mds(parity_code(c[0], c[1]), 1000 * c[0] + c[1]);
  run_mds(parity_code(5, 8), 5008);  // three rows: max_wrong = 2 answers as the one-shard rule
  Code z{6, 4, {0, 5, 7, 0, 2, 4,  //
                3, 0, 9, 0, 3, 6,  //
                1, 2, 0, 0, 0, 0,  //
                0, 0, 4, 0, 5, 10}};
  run_degenerate(z, 77);
  Code y{5, 5, {1, 2, 3, 0, 3,  //
                1, 3, 4, 0, 5,  //
                1, 4, 5, 1, 7,  //
                1, 5, 6, 0, 9,  //
                1, 6, 7, 0, 11}};
  run_degenerate(y, 78);
  if (failures) {
    printf("correct_rule_test: %d failures\n", failures);
    return 1;
  }
  printf("correct_rule_test ok\n");
  return 0;
}
