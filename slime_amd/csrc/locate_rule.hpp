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
// about k / p -- blamed on a third shard.
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

}  // namespace locate
}  // namespace slime
