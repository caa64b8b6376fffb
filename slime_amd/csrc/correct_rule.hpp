// The correct rule: what to write into the shards locate_rule.hpp names, from
// the column's syndromes.  One function set for the device
// (rs_correct_ragged_kernel.hpp) and the CPU (tests/cpp/correct_rule_test.cpp
// builds it with g++).  No HIP types; locate_rule.hpp supplies mul / sub / add
// and column_word.
//
// Notation as there: s_i = stored_i - computed_i (mod p), computed_i the row
// over the inputs AS THEY ARE STORED; h_a the column of slot a.  A wrong input a
// stored as x_a + e makes every computed_i too large by e c[i][a], so
// s = -e h_a: the right word is x_a + s_r / c[r][a] for any row r with
// c[r][a] != 0.  A wrong output row has s = e e_i: the right word is computed_i.
// For a pair {a, b} named by pair_slots, s = alpha h_a + beta h_b with
// alpha = A / D, beta = B / D from the first non-zero minor (p, q) exactly as
// pair_explains takes it; an input slot a becomes x_a + alpha, and an output row
// slot becomes the row over the corrected inputs, computed_i + alpha c[i][a] with
// a the pair's input (which equals stored_i - beta), or computed_i when both
// slots are rows.
//
// A Fix says what to ADD, per named slot: to the input's canonical residue for
// an input slot, to computed_i for an output row slot.  The caller reads the
// word or recomputes the row, adds, and stores the canonical result -- every
// row value must be taken BEFORE an input of the column is rewritten.
// `solved` false: the named input's coefficient column has no non-zero word (a
// slime_rs_plan_matrix plan; never one of the library's): nothing may be
// written and the column is unlocated.  pair_fix also returns it when it finds
// no non-zero minor, which is defensive only: pair_slots names no pair of
// dependent columns, so that branch is not reached behind it.
//
// The inverse is Fermat's, a^(p-2) over locate::mul -- 32 squarings and 30
// multiplies on a flagged column only; there is no inverse table on the plan.
#pragma once
#include <stdint.h>

#include "locate_rule.hpp"

namespace slime {
namespace correct {

using locate::add;
using locate::column_word;
using locate::mul;
using locate::sub;

// a^-1 mod p for canonical a != 0 (inv(0) == 0).
__host__ __device__ __forceinline__ uint32_t inv(uint32_t a) {
  uint32_t r = 1;
  for (uint32_t e = kP - 2; e; e >>= 1) {
    if (e & 1u) r = mul(r, a);
    a = mul(a, a);
  }
  return r;
}

struct Fix {
  bool solved;
  uint32_t da, db;  // what to add for the first and the second named slot
};

// Slot a named alone (Column::slot): s(i) the syndrome s_i, c(i, j) the plan's coefficient.
template <class S, class C>
__host__ __device__ __forceinline__ Fix single_fix(const S& s, const C& c, uint32_t k, uint32_t rows, uint32_t a) {
  if (a >= k) return Fix{true, 0, 0};
  for (uint32_t r = 0; r < rows; ++r) {
    const uint32_t h = canon(c(r, a));
    if (h != 0) return Fix{true, mul(s(r), inv(h)), 0};
  }
  return Fix{false, 0, 0};
}

// The pair {a, b}, a < b, named by pair_slots.
template <class S, class C>
__host__ __device__ __forceinline__ Fix pair_fix(const S& s, const C& c, uint32_t k, uint32_t rows, uint32_t a,
                                                 uint32_t b) {
  if (a >= k) return Fix{true, 0, 0};  // two output rows (b > a): both become their computed rows
  uint32_t p = 0, hap = 0;
  for (; p < rows; ++p)
    if ((hap = canon(c(p, a))) != 0) break;
  if (p == rows) return Fix{false, 0, 0};
  const uint32_t hbp = column_word(c, k, b, p);
  uint32_t q = 0, haq = 0, hbq = 0, D = 0;
  for (; q < rows; ++q) {
    if (q == p) continue;
    haq = column_word(c, k, a, q);
    hbq = column_word(c, k, b, q);
    D = sub(mul(hap, hbq), mul(haq, hbp));
    if (D != 0) break;
  }
  if (q == rows) return Fix{false, 0, 0};
  const uint32_t sp = s(p), sq = s(q), di = inv(D);
  const uint32_t alpha = mul(sub(mul(sp, hbq), mul(sq, hbp)), di);
  if (b < k) return Fix{true, alpha, mul(sub(mul(hap, sq), mul(haq, sp)), di)};
  return Fix{true, alpha, mul(alpha, canon(c(b - k, a)))};
}

}  // namespace correct
}  // namespace slime
