// Ragged verify for CDNA4 (gfx950): rs_verify.hip's question -- are the stored
// shards consistent with a plan? -- asked of a ragged batch in one launch
// (slime_rs_plan_verify_batch), and of a planned batch with a plan PER OBJECT
// out of a plan set's table (slime_rs_planset_verify_batch).  Nothing here is
// new arithmetic: the work comes from UnitWalk over the batch's unit list
// (rs_ragged_walk.hpp), the compare is load_tile / check_tile / check_columns
// and the accounting is Tally (rs_verify_kernel.hpp).  This file joins them.
//
// Forms (SET: the plan-set twin, one template):
//   k <= 16, 4-byte aligned src and cmp: rs_verify_ragged_kernel<K, W, R, ...>,
//     four columns a lane.  The batch's tile is 64 UB vectors a shard, UB the
//     apply launch's unroll for k; verify holds k + R vectors per unit, so a
//     wave takes a tile in steps of W <= UB vectors a lane (verify_step.hpp),
//     the last step clipped to the tile's end, and the software pipeline runs
//     over steps: the next step's k inputs and R stored rows are in flight
//     while this step's rows are compared.  Walks: dynamic (tickets), static
//     double-buffered, and static one step at a time (slime_rs_kernel_pipeline(0)),
//     chosen exactly as launch_apply_ragged chooses.
//   k > 16, or a base that is not 4-byte aligned: rs_verify_ragged_column_kernel,
//     one column per lane through check_columns<0> over the same unit list
//     (static walk).  Correct for any k, not fast.
//
// What travels with a step (StepRef), fixed when its loads are issued: the
// object's stored-row base and stride, its two result rows, the step's first
// vector and its clip, and the coefficient rows, output indices and row count
// of the object's plan.  After advance() the walk may stand on another object
// -- in the set form on another plan -- while the earlier step is still to be
// compared: the compare reads the StepRef only, never the walk (`w`, `cur`).
//
// Flush: a wave's Tally is flushed before a step of another object is
// tallied (its result pointer differs) and at the end of the walk; clean data
// issues no atomics, and a launch's atomics are bounded by (wave, run of
// steps of one object) pairs x rows.
//
// Tails: the {object, column} items past the objects' last whole vectors are
// strided over the grid, one per lane.  Neighbouring lanes hold different
// objects there, so Tally's lane-per-row scheme does not apply: a lane that
// finds a mismatch issues its own atomicAdd(1) and atomicMin for that row --
// at most three columns an object.
//
// Rows: a launch tallies at most 64 rows (one lane each); the host launches row
// blocks of 64 with the result, coefficient and output-index pointers moved on
// (the set form passes r0: each plan's block starts at its own offsets, and a
// unit whose plan has no row in the block is passed over without a load).
// Only plain C++ and vector atomics write memory.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "planset_table.hpp"
#include "rs_apply_kernel.hpp"
#include "rs_ragged_launch.hpp"
#include "rs_ragged_walk.hpp"
#include "rs_verify_kernel.hpp"
#include "rs_verify_ragged_kernel.hpp"  // the kernels' bodies: shared with rs_bytes_ragged.hip
#include "verify_step.hpp"

namespace slime {
namespace verify {

// The symbol forms' entry points: the shared bodies without a mapping.
#define SLIME_RVERIFY_SYMBOL_PARAMS                                                                                  \
  const uint8_t *__restrict__ in, const uint8_t *__restrict__ cmp, const Desc *__restrict__ descs,                   \
      const Unit *__restrict__ units, const Tail *__restrict__ tails, const uint32_t *__restrict__ coeff,            \
      const uint32_t *__restrict__ in_idx, const uint32_t *__restrict__ out_idx,                                     \
      unsigned long long *__restrict__ mism, unsigned long long *__restrict__ first, uint32_t nunits,                \
      uint64_t ntails, uint32_t rows, uint32_t k, uint32_t r0, uint32_t res_stride
#define SLIME_RVERIFY_SYMBOL_PASS \
  in, cmp, descs, units, tails, coeff, in_idx, out_idx, nullptr, mism, first, nunits, ntails, rows, k, r0, res_stride

template <int K, int W, int R, int UB, int C, int NC, bool DYN, bool PIPE, bool SET>
__global__ __launch_bounds__(kBlock) void rs_verify_ragged_kernel(SLIME_RVERIFY_SYMBOL_PARAMS,
                                                                  uint32_t* __restrict__ ticket) {
  constexpr bool BYTES = false;
  constexpr const uint32_t* mapping = nullptr;
#include "rs_verify_ragged_walk_body.hpp"
}

template <bool SET>
__global__ __launch_bounds__(kBlock) void rs_verify_ragged_column_kernel(SLIME_RVERIFY_SYMBOL_PARAMS,
                                                                         uint32_t tile_cols, uint32_t unit_tiles) {
  verify_ragged_columns<SET, false>(SLIME_RVERIFY_SYMBOL_PASS, tile_cols, unit_tiles);
}

#undef SLIME_RVERIFY_SYMBOL_PARAMS
#undef SLIME_RVERIFY_SYMBOL_PASS

}  // namespace verify

namespace {

using apply::kBlock;
using RowBlock = ragged::RowBlock<RaggedVerifyLaunch>;

#define SLIME_RVERIFY_ARGS(b, SET)                                                                                   \
  (const uint8_t*)(b).v.in, (const uint8_t*)(b).v.cmp, (b).v.w.desc, (b).v.w.units, (b).v.w.tails,                   \
      (SET) ? (b).v.p.table : (b).v.p.coeff + (uint64_t)(b).r0 * coeff_stride((b).v.w.k), (b).v.p.in_idx,           \
      (SET) ? (const uint32_t*)nullptr : (b).v.p.out_idx + (b).r0, (unsigned long long*)(b).v.mismatches + (b).r0,   \
      (unsigned long long*)(b).v.first + (b).r0, (b).v.w.nunits, (b).v.w.ntails, (SET) ? 0u : (b).rows_c, (b).v.w.k, \
      (SET) ? (b).r0 : 0u, (b).v.p.rows

template <int K, int R, bool SET>
hipError_t launch_vectors(const RowBlock& b, hipStream_t s) {
  constexpr int UB = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K), W = verify_step::width(K, R);
  // Static forms: fat waves one block a CU, thin ones (one vector a lane) four, as the uniform verify launch.
  return ragged::launch_scheduled(
      s, b.v.w.nunits, b.v.w.ntails, W == 1 ? 1024 : 256, [&](auto dyn, auto pipe, uint64_t blocks, uint32_t* set) {
        constexpr bool DYN = decltype(dyn)::value, PIPE = decltype(pipe)::value;
        hipLaunchKernelGGL((verify::rs_verify_ragged_kernel<K, W, R, UB, C, kQueueCounters, DYN, PIPE, SET>),
                           dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_RVERIFY_ARGS(b, SET), set);
        return hipGetLastError();
      });
}

template <int K>
hipError_t launch_rows(const RowBlock& b, hipStream_t s) {
  const bool set = b.v.p.table != nullptr;
  if (verify_step::stored_rows(b.rows_c) == 2)
    return set ? launch_vectors<K, 2, true>(b, s) : launch_vectors<K, 2, false>(b, s);
  return set ? launch_vectors<K, 4, true>(b, s) : launch_vectors<K, 4, false>(b, s);
}

hipError_t launch_columns(const RowBlock& b, hipStream_t s) {
  const uint64_t blocks = ragged::ragged_blocks(1024, b.v.w.nunits, b.v.w.ntails);
  if (b.v.p.table)
    hipLaunchKernelGGL(verify::rs_verify_ragged_column_kernel<true>, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                       SLIME_RVERIFY_ARGS(b, true), 256u * (uint32_t)b.v.w.U, (uint32_t)b.v.w.C);
  else
    hipLaunchKernelGGL(verify::rs_verify_ragged_column_kernel<false>, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                       SLIME_RVERIFY_ARGS(b, false), 256u * (uint32_t)b.v.w.U, (uint32_t)b.v.w.C);
  return hipGetLastError();
}

#undef SLIME_RVERIFY_ARGS

}  // namespace

hipError_t launch_verify_ragged(const RaggedVerifyLaunch& v, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (v.w.nobj == 0 || v.p.rows == 0) return hipSuccess;
  if (hipError_t e = launch_verify_init(v.mismatches, v.first, v.w.nobj * v.p.rows, s)) return e;
  if (v.w.nunits == 0 && v.w.ntails == 0) return hipSuccess;  // an empty batch: nothing but the initialisation
  const bool vec = v.w.k <= 16 && v.w.vec_ok;
  // The vector kernels are instantiated with the geometry of their K: the tables must be cut by it.
  if (vec && (v.w.U != ragged::unroll_for_k((int)v.w.k) || v.w.C != ragged::unit_tiles_for_k((int)v.w.k)))
    return hipErrorInvalidValue;
  return ragged::for_row_blocks(v, [&](const RowBlock& b) {
    if (!vec) return launch_columns(b, s);
    return ragged::with_k(v.w.k, [&](auto kc) { return launch_rows<decltype(kc)::value>(b, s); });
  });
}

}  // namespace slime
