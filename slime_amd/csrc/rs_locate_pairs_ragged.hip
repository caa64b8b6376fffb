// Pair locate for CDNA4 (gfx950): the ragged locate (rs_locate_ragged.hip) with
// the pair rule of locate_rule.hpp behind it, for plans of rows >= 4 --
// slime_rs_plan_locate_pairs_batch, slime_rs_locate_pairs_objects_batch and their
// plan-set twins.  A column with two wrong shards is named: it adds 1 to
// `counts` of both slots and takes part in `first` of both; everything else is
// the one-shard launch's answer, so results have the same shape and meaning.
//
// The bodies (rs_locate_pairs_kernel.hpp) are the one-shard bodies again over
// the same helpers: the fast path (flag_tile, the filter, the static walk, 1024
// blocks) is the same code.  The rare path differs.  A lane with a flagged
// column classifies it as before and on the way writes the column's `rows`
// syndromes into its slice of a dynamic-LDS strip of rows x kBlock words
// (strip[i][threadIdx.x]: a wave's accesses to one row are one conflict-free
// line) and keeps the d_i in a 64-bit register mask.  A column the one-shard rule leaves unlocated then
// runs the pair enumeration over the strip and the plan's coefficient rows --
// nothing per-row in registers, nothing in scratch.  tally_slots runs once per
// named slot (the lanes are in column order for both); tail items issue their
// own atomics for both slots.  The strip is 4 KiB a block at four rows and
// 60 KiB at 3/63, the widest plan a launch takes (k + rows <= 63).
//
// Sets: max_rows >= 4 is required; an object whose own plan has fewer than four
// rows takes the one-shard rule (set_slot: fewer than two, every wrong column
// unlocated).  R -- the stored rows a step carries -- is always 4 here.
// Only plain C++ and vector atomics write memory.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "rs_locate_pairs_kernel.hpp"
#include "rs_ragged_launch.hpp"
#include "verify_step.hpp"

namespace slime {
namespace locate {

extern __shared__ uint32_t pair_strip[];  // rows x kBlock syndromes, [i][threadIdx.x]

template <int K, int W, int UB, int C, bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_pairs_ragged_kernel(SLIME_RLOCATE_PARAMS) {
  locate_pairs_vectors<K, W, UB, C, false, BYTES>(SLIME_RLOCATE_PASS, pair_strip);
}

template <bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_pairs_ragged_column_kernel(SLIME_RLOCATE_PARAMS,
                                                                               uint32_t tile_cols,
                                                                               uint32_t unit_tiles) {
  locate_pairs_columns<false, BYTES>(SLIME_RLOCATE_PASS, tile_cols, unit_tiles, pair_strip);
}

// The plan-set entry points: the table as `coeff`, max_rows as `rows`, no index arrays.
#define SLIME_PLOCATE_PARAMS                                                                                      \
  const uint8_t *__restrict__ in, const uint8_t *__restrict__ cmp, const Desc *__restrict__ descs,                \
      const Unit *__restrict__ units, const Tail *__restrict__ tails, const uint32_t *__restrict__ table,         \
      const uint32_t *__restrict__ mapping, const unsigned long long *__restrict__ filter,                        \
      unsigned long long *__restrict__ counts, unsigned long long *__restrict__ first, uint32_t nunits,           \
      uint64_t ntails, uint32_t max_rows, uint32_t k
#define SLIME_PLOCATE_PASS \
  in, cmp, descs, units, tails, table, nullptr, nullptr, mapping, filter, counts, first, nunits, ntails, max_rows, k

template <int K, int W, int UB, int C, bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_pairs_planset_kernel(SLIME_PLOCATE_PARAMS) {
  locate_pairs_vectors<K, W, UB, C, true, BYTES>(SLIME_PLOCATE_PASS, pair_strip);
}

template <bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_pairs_planset_column_kernel(SLIME_PLOCATE_PARAMS,
                                                                                uint32_t tile_cols,
                                                                                uint32_t unit_tiles) {
  locate_pairs_columns<true, BYTES>(SLIME_PLOCATE_PASS, tile_cols, unit_tiles, pair_strip);
}

#undef SLIME_PLOCATE_PARAMS
#undef SLIME_PLOCATE_PASS

}  // namespace locate

namespace {

using apply::kBlock;

#define SLIME_RLOCATE_ARGS(v)                                                                                     \
  (const uint8_t*)(v).in, (const uint8_t*)(v).cmp, (v).w.desc, (v).w.units, (v).w.tails, (v).p.coeff,             \
      (v).p.in_idx, (v).p.out_idx, (v).mapping, (const unsigned long long*)(v).filter,                            \
      (unsigned long long*)(v).counts, (unsigned long long*)(v).first, (v).w.nunits, (v).w.ntails, (v).p.rows,    \
      (v).w.k
#define SLIME_PLOCATE_ARGS(v)                                                                                     \
  (const uint8_t*)(v).in, (const uint8_t*)(v).cmp, (v).w.desc, (v).w.units, (v).w.tails, (v).p.table,             \
      (v).mapping, (const unsigned long long*)(v).filter, (unsigned long long*)(v).counts,                        \
      (unsigned long long*)(v).first, (v).w.nunits, (v).w.ntails, (v).p.rows, (v).w.k

constexpr uint64_t kLocateBlocks = 1024;  // as rs_locate_ragged.hip: four blocks a CU

// The strip's bytes: one word per row (the plan's, or the set's widest) and thread of a block.
uint32_t strip_bytes(const RaggedLocateLaunch& v) { return v.p.rows * kBlock * (uint32_t)sizeof(uint32_t); }

template <int K, bool SET, bool BYTES>
hipError_t launch_vectors(const RaggedLocateLaunch& v, hipStream_t s) {
  constexpr int UB = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K), W = verify_step::width(K, 4);
  const dim3 grid((uint32_t)ragged::ragged_blocks(kLocateBlocks, v.w.nunits, v.w.ntails));
  if constexpr (SET)
    hipLaunchKernelGGL((locate::rs_locate_pairs_planset_kernel<K, W, UB, C, BYTES>), grid, dim3(kBlock),
                       strip_bytes(v), s, SLIME_PLOCATE_ARGS(v));
  else
    hipLaunchKernelGGL((locate::rs_locate_pairs_ragged_kernel<K, W, UB, C, BYTES>), grid, dim3(kBlock),
                       strip_bytes(v), s, SLIME_RLOCATE_ARGS(v));
  return hipGetLastError();
}

template <bool SET, bool BYTES>
hipError_t launch_columns(const RaggedLocateLaunch& v, hipStream_t s) {
  const dim3 grid((uint32_t)ragged::ragged_blocks(kLocateBlocks, v.w.nunits, v.w.ntails));
  const uint32_t tile_cols = 256u * (uint32_t)v.w.U, unit_tiles = (uint32_t)v.w.C;
  if constexpr (SET)
    hipLaunchKernelGGL(locate::rs_locate_pairs_planset_column_kernel<BYTES>, grid, dim3(kBlock), strip_bytes(v), s,
                       SLIME_PLOCATE_ARGS(v), tile_cols, unit_tiles);
  else
    hipLaunchKernelGGL(locate::rs_locate_pairs_ragged_column_kernel<BYTES>, grid, dim3(kBlock), strip_bytes(v), s,
                       SLIME_RLOCATE_ARGS(v), tile_cols, unit_tiles);
  return hipGetLastError();
}

#undef SLIME_RLOCATE_ARGS
#undef SLIME_PLOCATE_ARGS

template <bool SET>
hipError_t launch_form(const RaggedLocateLaunch& v, bool vec, hipStream_t s) {
  if (!vec) return v.mapping ? launch_columns<SET, true>(v, s) : launch_columns<SET, false>(v, s);
  return ragged::with_k(v.w.k, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    return v.mapping ? launch_vectors<K, SET, true>(v, s) : launch_vectors<K, SET, false>(v, s);
  });
}

}  // namespace

hipError_t launch_locate_pairs_ragged(const RaggedLocateLaunch& v, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (v.w.nobj == 0) return hipSuccess;
  // k + rows <= 63 also bounds the strip: at most 60 rows x 256 threads x 4 bytes = 60 KiB.
  if (v.p.rows < locate::kPairRows || v.w.k + v.p.rows > locate::kMaxSlots) return hipErrorInvalidValue;
  if (hipError_t e = launch_verify_init(v.counts, v.first, v.w.nobj * (v.w.k + v.p.rows + 1), s)) return e;
  if (v.w.nunits == 0 && v.w.ntails == 0) return hipSuccess;  // an empty batch: nothing but the initialisation
  const bool vec = v.w.k <= 16 && v.w.vec_ok;
  // The vector kernels are instantiated with the geometry of their K: the tables must be cut by it.
  if (vec && (v.w.U != ragged::unroll_for_k((int)v.w.k) || v.w.C != ragged::unit_tiles_for_k((int)v.w.k)))
    return hipErrorInvalidValue;
  return v.p.table ? launch_form<true>(v, vec, s) : launch_form<false>(v, vec, s);  // a set: a plan per object
}

}  // namespace slime
