// Ragged locate for CDNA4 (gfx950): after a scrub (rs_verify_ragged.hip) said
// WHICH ROWS of an object disagree, this launch says WHICH SHARD is wrong, per
// column, by the rule of locate_rule.hpp -- slime_rs_plan_locate_batch over
// symbols, slime_rs_locate_objects_batch over stored chunk bytes.  Results:
// counts[o][slot] columns blamed on slot, first[o][slot] the lowest of them;
// slots are the plan's k inputs, its rows, then `unlocated`.
//
// Plan sets (SET, one template): the same launch over a PLANNED batch, every
// object classified with its own plan of a set -- slime_rs_planset_locate_batch
// and slime_rs_planset_locate_objects_batch.  A degraded object is scrubbed
// (rs_verify_ragged.hip, the SET forms) and located from its own survivor set:
// its plan reads `k` present shards and checks the remaining present ones.
// Results are nobj x (k + max_rows + 1): slot j < k is the object's plan's
// input j, slot k + i (i < the plan's rows) its output row i, slots past the
// plan's rows keep their initial values, and `unlocated` is slot k + max_rows
// for every object.  Objects whose plan has one row report every mismatching
// column as unlocated (locate_rule.hpp, set_slot).  What SET adds per object is
// one plan record (two dependent scalar loads) and, for k <= 16, one 16-dword
// line of input indices, taken when the walk enters the object; R -- the stored
// rows a step carries -- is chosen from max_rows, and the filter is the nobj x
// max_rows counts of a plan-set verify.
//
// Fast path -- verify's: the work comes from UnitWalk over the batch's unit
// list (rs_ragged_walk.hpp), a tile goes in verify's steps (verify_step.hpp),
// load_tile loads a step and dot4 computes its rows.  Instead of a tally per
// row, every row's word deltas are OR-ed into a per-lane mask across all row
// blocks (flag_tile): clean data costs verify's loads and math plus that OR,
// with no atomics and no stores.  A unit whose object the filter clears (all
// of a preceding verify's counts zero, read here on the device) is passed over
// before any load.
//
// Rare path -- only when a ballot of the mask is non-zero: a lane with a
// flagged column re-reads that column's k inputs and `rows` stored words (just
// loaded: cache hits) and classifies it (classify_column), keeping s_0, the
// count of mismatching rows, the last such row and a 64-bit mask of the inputs
// that still satisfy the relation -- no per-row arrays, nothing in scratch.
//
// Tallying: a wave's classified columns are folded slot by slot (ballot /
// readlane over the distinct slots present) into verify's Tally with lane =
// slot -- hence k + rows <= 63 -- and flushed with atomicAdd / atomicMin when
// the wave moves to another object and at the end of the walk.  Tail items
// (L % 4 columns an object) classify one column a lane and issue their own
// atomics.
//
// Pair locate (PAIRS, one template; v.pairs): the same launch with the pair
// rule of locate_rule.hpp behind the one-shard rule, for plans of rows >= 4 --
// slime_rs_plan_locate_pairs_batch, slime_rs_locate_pairs_objects_batch and their
// plan-set twins.  A column with two wrong shards is named: it adds 1 to
// `counts` of both slots and takes part in `first` of both; everything else is
// the one-shard launch's answer, so results have the same shape and meaning.
// The fast path is the same code; the rare path differs.  A lane with a flagged
// column classifies it as before and on the way writes the column's `rows`
// syndromes into its slice of a dynamic-LDS strip of rows x kBlock words
// (strip[i][threadIdx.x]: a wave's accesses to one row are one conflict-free
// line) and keeps the d_i in a 64-bit register mask.  A column the one-shard
// rule leaves unlocated then runs the pair enumeration over the strip and the
// plan's coefficient rows -- nothing per-row in registers, nothing in scratch.
// tally_slots runs once per named slot (the lanes are in column order for
// both); tail items issue their own atomics for both slots.  The strip is 4 KiB
// a block at four rows and 60 KiB at 3/63, the widest plan a launch takes
// (k + rows <= 63); the one-shard kernels use no LDS.  Sets: max_rows >= 4 is
// required; an object whose own plan has fewer than four rows takes the
// one-shard rule (set_slot: fewer than two, every wrong column unlocated).
// R is always 4 with PAIRS.
//
// Forms (rs_locate_planset_*: the SET twins, rs_locate_pairs_*: the PAIRS
// twins of both, the same bodies):
//   k <= 16, 4-byte aligned src and cmp: rs_locate_ragged_kernel<K, W, R, ...>,
//     four columns a lane, symbols and bytes from one body (BYTES).
//   17 <= k (k + rows <= 63), or a base that is not 4-byte aligned:
//     rs_locate_ragged_column_kernel, one column a lane over the same unit list.
// Walk: static, one step at a time, in every schedule / pipeline mode (so the
// modes cannot differ); latency is hidden by occupancy, four blocks a CU.
// Only plain C++ and vector atomics write memory.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "rs_locate_ragged_kernel.hpp"
#include "rs_ragged_launch.hpp"
#include "verify_step.hpp"

namespace slime {
namespace locate {

extern __shared__ uint32_t pair_strip[];  // PAIRS: rows x kBlock syndromes, [i][threadIdx.x]

template <int K, int W, int R, int UB, int C, bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_ragged_kernel(SLIME_RLOCATE_PARAMS) {
  locate_vectors<false, K, W, R, UB, C, false, BYTES>(SLIME_RLOCATE_PASS, nullptr);
}

template <bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_ragged_column_kernel(SLIME_RLOCATE_PARAMS, uint32_t tile_cols,
                                                                         uint32_t unit_tiles) {
  locate_columns<false, false, BYTES>(SLIME_RLOCATE_PASS, tile_cols, unit_tiles, nullptr);
}

template <int K, int W, int UB, int C, bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_pairs_ragged_kernel(SLIME_RLOCATE_PARAMS) {
  locate_vectors<true, K, W, 4, UB, C, false, BYTES>(SLIME_RLOCATE_PASS, pair_strip);
}

template <bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_pairs_ragged_column_kernel(SLIME_RLOCATE_PARAMS,
                                                                               uint32_t tile_cols,
                                                                               uint32_t unit_tiles) {
  locate_columns<true, false, BYTES>(SLIME_RLOCATE_PASS, tile_cols, unit_tiles, pair_strip);
}

// The plan-set entry points: the shared bodies with the table as `coeff`, max_rows as `rows` and
// no index arrays.
#define SLIME_PLOCATE_PARAMS                                                                                      \
  const uint8_t *__restrict__ in, const uint8_t *__restrict__ cmp, const Desc *__restrict__ descs,                \
      const Unit *__restrict__ units, const Tail *__restrict__ tails, const uint32_t *__restrict__ table,         \
      const uint32_t *__restrict__ mapping, const unsigned long long *__restrict__ filter,                        \
      unsigned long long *__restrict__ counts, unsigned long long *__restrict__ first, uint32_t nunits,           \
      uint64_t ntails, uint32_t max_rows, uint32_t k
#define SLIME_PLOCATE_PASS \
  in, cmp, descs, units, tails, table, nullptr, nullptr, mapping, filter, counts, first, nunits, ntails, max_rows, k

template <int K, int W, int R, int UB, int C, bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_planset_kernel(SLIME_PLOCATE_PARAMS) {
  locate_vectors<false, K, W, R, UB, C, true, BYTES>(SLIME_PLOCATE_PASS, nullptr);
}

template <bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_planset_column_kernel(SLIME_PLOCATE_PARAMS, uint32_t tile_cols,
                                                                          uint32_t unit_tiles) {
  locate_columns<false, true, BYTES>(SLIME_PLOCATE_PASS, tile_cols, unit_tiles, nullptr);
}

template <int K, int W, int UB, int C, bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_pairs_planset_kernel(SLIME_PLOCATE_PARAMS) {
  locate_vectors<true, K, W, 4, UB, C, true, BYTES>(SLIME_PLOCATE_PASS, pair_strip);
}

template <bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_pairs_planset_column_kernel(SLIME_PLOCATE_PARAMS,
                                                                                uint32_t tile_cols,
                                                                                uint32_t unit_tiles) {
  locate_columns<true, true, BYTES>(SLIME_PLOCATE_PASS, tile_cols, unit_tiles, pair_strip);
}

#undef SLIME_PLOCATE_PARAMS
#undef SLIME_PLOCATE_PASS

}  // namespace locate

namespace {

using apply::kBlock;

// One per kernel signature; (v).p.rows is the plan's rows or the set's max_rows.
#define SLIME_RLOCATE_ARGS(v)                                                                                     \
  (const uint8_t*)(v).in, (const uint8_t*)(v).cmp, (v).w.desc, (v).w.units, (v).w.tails, (v).p.coeff,             \
      (v).p.in_idx, (v).p.out_idx, (v).mapping, (const unsigned long long*)(v).filter,                            \
      (unsigned long long*)(v).counts, (unsigned long long*)(v).first, (v).w.nunits, (v).w.ntails, (v).p.rows,    \
      (v).w.k
#define SLIME_PLOCATE_ARGS(v)                                                                                     \
  (const uint8_t*)(v).in, (const uint8_t*)(v).cmp, (v).w.desc, (v).w.units, (v).w.tails, (v).p.table,             \
      (v).mapping, (const unsigned long long*)(v).filter, (unsigned long long*)(v).counts,                        \
      (unsigned long long*)(v).first, (v).w.nunits, (v).w.ntails, (v).p.rows, (v).w.k

constexpr uint64_t kLocateBlocks = 1024;  // four blocks a CU: the static walk hides latency by occupancy

// The dynamic LDS of a block.  PAIRS: the strip, one word per row (the plan's, or the set's widest)
// and thread; k + rows <= 63 bounds it at 60 rows x 256 threads x 4 bytes = 60 KiB.
template <bool PAIRS>
uint32_t strip_bytes(const RaggedLocateLaunch& v) {
  return PAIRS ? v.p.rows * kBlock * (uint32_t)sizeof(uint32_t) : 0;
}

template <int K, int R, bool PAIRS, bool SET, bool BYTES>
hipError_t launch_vectors(const RaggedLocateLaunch& v, hipStream_t s) {
  static_assert(!PAIRS || R == 4, "the pair kernels carry four stored rows a step");
  constexpr int UB = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K), W = verify_step::width(K, R);
  const dim3 grid((uint32_t)ragged::ragged_blocks(kLocateBlocks, v.w.nunits, v.w.ntails));
  const uint32_t lds = strip_bytes<PAIRS>(v);
  if constexpr (PAIRS && SET)
    hipLaunchKernelGGL((locate::rs_locate_pairs_planset_kernel<K, W, UB, C, BYTES>), grid, dim3(kBlock), lds, s,
                       SLIME_PLOCATE_ARGS(v));
  else if constexpr (PAIRS)
    hipLaunchKernelGGL((locate::rs_locate_pairs_ragged_kernel<K, W, UB, C, BYTES>), grid, dim3(kBlock), lds, s,
                       SLIME_RLOCATE_ARGS(v));
  else if constexpr (SET)
    hipLaunchKernelGGL((locate::rs_locate_planset_kernel<K, W, R, UB, C, BYTES>), grid, dim3(kBlock), lds, s,
                       SLIME_PLOCATE_ARGS(v));
  else
    hipLaunchKernelGGL((locate::rs_locate_ragged_kernel<K, W, R, UB, C, BYTES>), grid, dim3(kBlock), lds, s,
                       SLIME_RLOCATE_ARGS(v));
  return hipGetLastError();
}

// R -- the stored rows a step carries -- from the plan's rows or the set's max_rows; always 4
// with PAIRS, whose launches have rows >= 4.
template <int K, bool PAIRS, bool SET>
hipError_t launch_rows(const RaggedLocateLaunch& v, hipStream_t s) {
  const bool bytes = v.mapping != nullptr;
  if constexpr (!PAIRS)
    if (verify_step::stored_rows(v.p.rows) == 2)
      return bytes ? launch_vectors<K, 2, false, SET, true>(v, s) : launch_vectors<K, 2, false, SET, false>(v, s);
  return bytes ? launch_vectors<K, 4, PAIRS, SET, true>(v, s) : launch_vectors<K, 4, PAIRS, SET, false>(v, s);
}

template <bool PAIRS, bool SET, bool BYTES>
hipError_t launch_columns(const RaggedLocateLaunch& v, hipStream_t s) {
  const dim3 grid((uint32_t)ragged::ragged_blocks(kLocateBlocks, v.w.nunits, v.w.ntails));
  const uint32_t tile_cols = 256u * (uint32_t)v.w.U, unit_tiles = (uint32_t)v.w.C, lds = strip_bytes<PAIRS>(v);
  if constexpr (PAIRS && SET)
    hipLaunchKernelGGL(locate::rs_locate_pairs_planset_column_kernel<BYTES>, grid, dim3(kBlock), lds, s,
                       SLIME_PLOCATE_ARGS(v), tile_cols, unit_tiles);
  else if constexpr (PAIRS)
    hipLaunchKernelGGL(locate::rs_locate_pairs_ragged_column_kernel<BYTES>, grid, dim3(kBlock), lds, s,
                       SLIME_RLOCATE_ARGS(v), tile_cols, unit_tiles);
  else if constexpr (SET)
    hipLaunchKernelGGL(locate::rs_locate_planset_column_kernel<BYTES>, grid, dim3(kBlock), lds, s,
                       SLIME_PLOCATE_ARGS(v), tile_cols, unit_tiles);
  else
    hipLaunchKernelGGL(locate::rs_locate_ragged_column_kernel<BYTES>, grid, dim3(kBlock), lds, s,
                       SLIME_RLOCATE_ARGS(v), tile_cols, unit_tiles);
  return hipGetLastError();
}

#undef SLIME_RLOCATE_ARGS
#undef SLIME_PLOCATE_ARGS

template <bool PAIRS, bool SET>
hipError_t launch_form(const RaggedLocateLaunch& v, bool vec, hipStream_t s) {
  if (!vec) return v.mapping ? launch_columns<PAIRS, SET, true>(v, s) : launch_columns<PAIRS, SET, false>(v, s);
  return ragged::with_k(v.w.k, [&](auto kc) { return launch_rows<decltype(kc)::value, PAIRS, SET>(v, s); });
}

}  // namespace

hipError_t launch_locate_ragged(const RaggedLocateLaunch& v, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (v.w.nobj == 0) return hipSuccess;
  if (v.p.rows < (v.pairs ? locate::kPairRows : 2u) || v.w.k + v.p.rows > locate::kMaxSlots)
    return hipErrorInvalidValue;
  if (hipError_t e = launch_verify_init(v.counts, v.first, v.w.nobj * (v.w.k + v.p.rows + 1), s)) return e;
  if (v.w.nunits == 0 && v.w.ntails == 0) return hipSuccess;  // an empty batch: nothing but the initialisation
  const bool vec = v.w.k <= 16 && v.w.vec_ok;
  // The vector kernels are instantiated with the geometry of their K: the tables must be cut by it.
  if (vec && (v.w.U != ragged::unroll_for_k((int)v.w.k) || v.w.C != ragged::unit_tiles_for_k((int)v.w.k)))
    return hipErrorInvalidValue;
  // a set: a plan per object
  if (v.pairs) return v.p.table ? launch_form<true, true>(v, vec, s) : launch_form<true, false>(v, vec, s);
  return v.p.table ? launch_form<false, true>(v, vec, s) : launch_form<false, false>(v, vec, s);
}

}  // namespace slime
