// The locate rule: which shard of a column is wrong, from the column's
// syndrome.  One function set for the device (rs_locate_ragged_kernel.hpp) and
// the CPU (tests/cpp/locate_rule_test.cpp builds it with g++), so the CPU tests
// exactly what the device runs.  No HIP types; gfp.hpp supplies fold96 / canon.
//
// A plan has k inputs and rows >= 2 output rows with coefficients c[i][j].  For
// one column, with computed_i the canonical residue of row i over the inputs
// as they are stored and stored_i the stored word of row i:
//   d_i = stored_i is not bit-identical to computed_i   (verify's rule: a
//         stored p + 3 where 3 is computed counts)
//   s_i = (stored_i mod p - computed_i) mod p            (the syndrome)
// The column is
//   clean            no d_i set                                   -> kNoSlot
//   output row i     exactly one d_i set                          -> slot k + i
//   input j          J = { j : s_0 != 0 and for all i
//                          s_i c[0][j] == s_0 c[i][j] (mod p) },
//                    |J| == 1                                     -> slot j
//   unlocated        anything else                                -> slot k + rows
// Why no inverse: a wrong input j adds delta c[i][j] to every row's syndrome,
// so s_i / s_0 = c[i][j] / c[0][j]; cross-multiplied the test needs products
// only, and holds for any delta.  For an MDS code's plans every 2 x 2 minor of
// the rows is non-zero, so two inputs never pass together: one wrong shard in
// a column is always named.  Two or more wrong shards in one column are beyond
// what `rows` syndromes decide: the column is unlocated, or -- with probability
// about k / p -- blamed on a third shard.  With rows >= 4 the pair rule at the
// end of this file names two wrong shards of a column, behind this rule.
//
// Column keeps s_0, the count of d_i, the last set i and a 64-bit mask of the
// inputs that still pass: no per-row arrays, rows fed one at a time.
#pragma once
#include <stdint.h>

#include "gfp.hpp"

namespace slime {
namespace locate {

constexpr uint32_t kMaxSlots = 63;         // k + rows: one result slot per lane of a wave, plus `unlocated`
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;  // a clean column

// a * b mod p for any uint32 a, b: the product fits fold96's low 64 bits.
__host__ __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) { return fold96((uint64_t)a * b, 0u); }
// (a - b) mod p for canonical a, b.
__host__ __device__ __forceinline__ uint32_t sub(uint32_t a, uint32_t b) { return a >= b ? a - b : a + (kP - b); }

struct Column {
  uint64_t cand;  // bit j: input j still satisfies the relation in every row so far
  uint32_t s0, nd, last;
  __host__ __device__ __forceinline__ void begin(uint32_t k) {
    cand = k >= 64 ? ~0ull : (1ull << k) - 1;
    s0 = nd = last = 0;
  }
  // Row i (fed in order from 0): its canonical residue, the stored symbol (any
  // uint32), and coefficient rows 0 and i of the plan (k words each).
  __host__ __device__ __forceinline__ void row(uint32_t i, uint32_t computed, uint32_t stored, const uint32_t* c0,
                                               const uint32_t* ci) {
    if (stored != computed) {
      ++nd;
      last = i;
    }
    const uint32_t s = sub(canon(stored), computed);
    if (i == 0) {
      s0 = s;
      if (s == 0) cand = 0;
      return;
    }
    for (uint64_t left = cand; left; left &= left - 1) {
      const int j = __builtin_ctzll(left);
      if (mul(s, c0[j]) != mul(s0, ci[j])) cand &= ~(1ull << j);
    }
  }
  __host__ __device__ __forceinline__ uint32_t slot(uint32_t k, uint32_t rows) const {
    if (nd == 0) return kNoSlot;
    if (nd == 1) return k + last;
    if (cand != 0 && (cand & (cand - 1)) == 0) return (uint32_t)__builtin_ctzll(cand);
    return k + rows;
  }
  // The slot in a plan SET's result row (set_slot below): this column's plan has `rows` rows,
  // the set's widest has max_rows.
  __host__ __device__ __forceinline__ uint32_t slot_in_set(uint32_t k, uint32_t rows, uint32_t max_rows) const;
};

// A plan set's result row has k + max_rows + 1 slots for every object, whatever its own plan's
// row count: inputs and rows keep slot()'s numbers, `unlocated` is always slot k + max_rows (one
// column of the result means the same for every object), slots k + rows .. k + max_rows - 1 are
// never named.  `slot` is Column::slot(k, rows) of the object's own plan.  A plan of ONE row
// cannot tell an input from its output -- slot() would name the row -- so every mismatching
// column of such an object is unlocated: the answer is per object, where the single-plan entry
// point refuses rows < 2 outright.
__host__ __device__ __forceinline__ uint32_t set_slot(uint32_t slot, uint32_t k, uint32_t rows, uint32_t max_rows) {
  if (slot == kNoSlot) return kNoSlot;
  if (rows < 2 || slot == k + rows) return k + max_rows;
  return slot;
}
__host__ __device__ __forceinline__ uint32_t Column::slot_in_set(uint32_t k, uint32_t rows, uint32_t max_rows) const {
  return set_slot(slot(k, rows), k, rows, max_rows);
}

// ---- The pair rule: two wrong shards in one column, from rows >= 4 syndromes ----
// h_a, the column of slot a, is (c[0][a], ..., c[rows-1][a]) for an input a < k and the unit
// vector e_i for the output row slot k + i.  A column is classified in this order:
//   1. Column::slot names a slot, or says clean: that is the answer.
//   2. rows < 4: unlocated, as Column::slot said.
//   3. exactly two d_i set: those two output rows (bit-wise, as d_i is: a stored p + 3 where 3
//      is computed counts).
//   4. P = the unordered pairs {a, b} of slots with h_a, h_b independent and
//      s = alpha h_a + beta h_b for some alpha != 0, beta != 0.  |P| == 1: both slots are named;
//      anything else is unlocated.
// Whether a pair explains s is decided without an inverse (pair_explains): from any non-zero
// minor D = h_a[p] h_b[q] - h_a[q] h_b[p], Cramer's numerators A = s_p h_b[q] - s_q h_b[p] and
// B = h_a[p] s_q - h_a[q] s_p give alpha = A / D, beta = B / D, so the pair explains s iff
// A != 0, B != 0 and D s_i == A h_a[i] + B h_b[i] in every row i.  The outcome does not depend
// on which non-zero minor is taken (alpha and beta are unique for independent columns), so the
// search takes the first row p with h_a[p] != 0 and the first q != p with D != 0 -- if h_a[p]
// != 0 and no such q exists, h_b is a multiple of h_a -- which costs `rows` steps where the
// lexicographic scan over row pairs costs rows^2.  Columns without a non-zero minor never explain.
// For an MDS code's plans (distance rows + 1 >= 5) two explanations of weight <= 2 would add up
// to a codeword of weight <= 4: one or two wrong shards in a column are always named.  Three or
// more are unlocated, or blamed on a wrong pair with probability about
// (k + rows)^2 / (2 p^(rows - 2)) per such column.  The enumeration stops at the second
// explaining pair -- the answer is then unlocated whatever follows -- and takes no other
// shortcut: the result equals the statement above for every matrix.
constexpr uint32_t kPairRows = 4;  // the fewest rows that decide two wrong shards

struct Slots {
  uint32_t a, b;  // a: clean, a slot or unlocated, as Column::slot; b: a pair's second slot, else kNoSlot
};

// (a + b) mod p for canonical a, b.
__host__ __device__ __forceinline__ uint32_t add(uint32_t a, uint32_t b) {
  const uint64_t t = (uint64_t)a + b;
  return (uint32_t)(t >= kP ? t - kP : t);
}

// h_a[i], canonical; c(i, j) is the plan's coefficient c[i][j] (any uint32).
template <class C>
__host__ __device__ __forceinline__ uint32_t column_word(const C& c, uint32_t k, uint32_t a, uint32_t i) {
  return a < k ? canon(c(i, a)) : (a - k == i ? 1u : 0u);
}

// true iff s = alpha h_a + beta h_b with alpha != 0, beta != 0 and h_a, h_b independent.  s(i) is
// the column's syndrome s_i (canonical).
template <class S, class C>
__host__ __device__ __forceinline__ bool pair_explains(const S& s, const C& c, uint32_t k, uint32_t rows, uint32_t a,
                                                       uint32_t b) {
  uint32_t p = 0, hap = 0;
  if (a >= k) {
    p = a - k;
    hap = 1;
  } else {
    for (; p < rows; ++p)
      if ((hap = canon(c(p, a))) != 0) break;
    if (p == rows) return false;  // h_a == 0
  }
  const uint32_t hbp = column_word(c, k, b, p);
  uint32_t q = 0, haq = 0, hbq = 0, D = 0;
  for (; q < rows; ++q) {
    if (q == p) continue;
    haq = column_word(c, k, a, q);
    hbq = column_word(c, k, b, q);
    D = sub(mul(hap, hbq), mul(haq, hbp));
    if (D != 0) break;
  }
  if (q == rows) return false;  // h_b is a multiple of h_a
  const uint32_t sp = s(p), sq = s(q);
  const uint32_t A = sub(mul(sp, hbq), mul(sq, hbp));
  const uint32_t B = sub(mul(hap, sq), mul(haq, sp));
  if (A == 0 || B == 0) return false;
  for (uint32_t i = 0; i < rows; ++i) {
    if (i == p || i == q) continue;  // rows p and q hold by construction
    if (mul(D, s(i)) != add(mul(A, column_word(c, k, a, i)), mul(B, column_word(c, k, b, i)))) return false;
  }
  return true;
}

// The pair rule on one column.  single: Column::slot(k, rows) of the column; dmask: bit i set iff
// d_i (rows <= 64); s, c: accessors as above, read only when the column reaches case 4.
template <class S, class C>
__host__ __device__ __forceinline__ Slots pair_slots(uint32_t single, uint64_t dmask, const S& s, const C& c,
                                                     uint32_t k, uint32_t rows) {
  if (single != k + rows || rows < kPairRows) return Slots{single, kNoSlot};
  const uint64_t high = dmask & (dmask - 1);  // dmask without its lowest bit
  if (high != 0 && (high & (high - 1)) == 0)
    return Slots{k + (uint32_t)__builtin_ctzll(dmask), k + (uint32_t)__builtin_ctzll(high)};
  Slots found{k + rows, kNoSlot};
  uint32_t n = 0;
  for (uint32_t a = 0; a + 1 < k + rows; ++a)
    for (uint32_t b = a + 1; b < k + rows; ++b)
      if (pair_explains(s, c, k, rows, a, b)) {
        if (++n > 1) return Slots{k + rows, kNoSlot};
        found = Slots{a, b};
      }
  return found;
}

// A pair's slots in a plan set's result row: set_slot on the first (the second is a named slot of
// the object's own plan, or kNoSlot, and keeps its number).
__host__ __device__ __forceinline__ Slots set_slots(Slots p, uint32_t k, uint32_t rows, uint32_t max_rows) {
  return Slots{set_slot(p.a, k, rows, max_rows), p.b};
}

}  // namespace locate
}  // namespace slime
