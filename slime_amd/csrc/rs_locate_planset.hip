// Plan-set locate for CDNA4 (gfx950): the ragged locate (rs_locate_ragged.hip)
// over a PLANNED batch, every object classified with its own plan of a set --
// slime_rs_planset_locate_batch over symbols,
// slime_rs_planset_locate_objects_batch over stored chunk bytes.  A degraded
// object is scrubbed (rs_verify_ragged.hip, the SET forms) and located from its
// own survivor set: its plan reads `k` present shards and checks the remaining
// present ones.
//
// Results: counts / first of nobj x (k + max_rows + 1).  Slot j < k is the
// object's plan's input j, slot k + i (i < the plan's rows) its output row i,
// slots past the plan's rows keep their initial values, and `unlocated` is slot
// k + max_rows for every object.  Objects whose plan has one row report every
// mismatching column as unlocated (locate_rule.hpp, set_slot).
//
// Scheme, forms, walk and tallying are rs_locate_ragged.hip's; the bodies are
// in rs_locate_planset_kernel.hpp.  What is added per object is one plan
// record (two dependent scalar loads) and, for k <= 16, one 16-dword line of
// input indices, taken when the walk enters the object; R -- the stored rows a
// step carries -- is chosen from max_rows.  The filter is the nobj x max_rows
// counts of a plan-set verify.  Only plain C++ and vector atomics write memory.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "rs_locate_planset_kernel.hpp"
#include "rs_ragged_launch.hpp"
#include "verify_step.hpp"

namespace slime {
namespace locate {

template <int K, int W, int R, int UB, int C, bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_planset_kernel(SLIME_PLOCATE_PARAMS) {
  locate_planset_vectors<K, W, R, UB, C, BYTES>(SLIME_PLOCATE_PASS);
}

template <bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_locate_planset_column_kernel(SLIME_PLOCATE_PARAMS, uint32_t tile_cols,
                                                                          uint32_t unit_tiles) {
  locate_planset_columns<BYTES>(SLIME_PLOCATE_PASS, tile_cols, unit_tiles);
}

}  // namespace locate

namespace {

using apply::kBlock;

#define SLIME_PLOCATE_ARGS(v)                                                                                  \
  (const uint8_t*)(v).in, (const uint8_t*)(v).cmp, (v).w.desc, (v).w.units, (v).w.tails, (v).p.table,          \
      (v).mapping, (const unsigned long long*)(v).filter, (unsigned long long*)(v).counts,                     \
      (unsigned long long*)(v).first, (v).w.nunits, (v).w.ntails, (v).p.rows, (v).w.k

constexpr uint64_t kLocateBlocks = 1024;  // rs_locate_ragged.hip's: four blocks a CU

template <int K, int R, bool BYTES>
hipError_t launch_vectors(const RaggedLocateLaunch& v, hipStream_t s) {
  constexpr int UB = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K), W = verify_step::width(K, R);
  const uint64_t blocks = ragged::ragged_blocks(kLocateBlocks, v.w.nunits, v.w.ntails);
  hipLaunchKernelGGL((locate::rs_locate_planset_kernel<K, W, R, UB, C, BYTES>), dim3((uint32_t)blocks), dim3(kBlock),
                     0, s, SLIME_PLOCATE_ARGS(v));
  return hipGetLastError();
}

template <int K>
hipError_t launch_rows(const RaggedLocateLaunch& v, hipStream_t s) {
  const bool bytes = v.mapping != nullptr;
  if (verify_step::stored_rows(v.p.rows) == 2)
    return bytes ? launch_vectors<K, 2, true>(v, s) : launch_vectors<K, 2, false>(v, s);
  return bytes ? launch_vectors<K, 4, true>(v, s) : launch_vectors<K, 4, false>(v, s);
}

hipError_t launch_columns(const RaggedLocateLaunch& v, hipStream_t s) {
  const uint64_t blocks = ragged::ragged_blocks(kLocateBlocks, v.w.nunits, v.w.ntails);
  if (v.mapping)
    hipLaunchKernelGGL(locate::rs_locate_planset_column_kernel<true>, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                       SLIME_PLOCATE_ARGS(v), 256u * (uint32_t)v.w.U, (uint32_t)v.w.C);
  else
    hipLaunchKernelGGL(locate::rs_locate_planset_column_kernel<false>, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                       SLIME_PLOCATE_ARGS(v), 256u * (uint32_t)v.w.U, (uint32_t)v.w.C);
  return hipGetLastError();
}

#undef SLIME_PLOCATE_ARGS

}  // namespace

// v.p.table: the set's table; v.p.rows: its max_rows.  launch_locate_ragged has initialised the
// results and checked the geometry.
hipError_t launch_locate_planset(const RaggedLocateLaunch& v, hipStream_t s) {
  const bool vec = v.w.k <= 16 && v.w.vec_ok;
  if (!vec) return launch_columns(v, s);
  return ragged::with_k(v.w.k, [&](auto kc) { return launch_rows<decltype(kc)::value>(v, s); });
}

}  // namespace slime
