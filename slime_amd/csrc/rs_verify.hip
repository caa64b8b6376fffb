// Device-side verify for CDNA4 (gfx950): are the stored shards of a batch
// consistent with a plan?  For every object o and output row i the kernels
// report how many columns would change if the plan were executed into the
// compared buffer, and the lowest such column.  A column mismatches iff the
// canonical residue sum_j coeff[i][j] * in[j][b] mod p is not bit-identical to
// the stored word (so a stored non-canonical p+3 where 3 is computed counts).
//
// Shape of the work: the apply kernels' (rs_apply_kernel.hpp) with the stores
// replaced by loads -- a lane owns 4 consecutive columns, loads them from the
// k input shards AND from the `rows` stored rows, runs the same dot4 against
// scalar-loaded coefficient rows and compares.  Traffic is that of the encode
// launch, all reads; nothing is written but the two result arrays, and no
// scratch is used.
//
// Stored rows travel with the tile: R stored rows (R = 2 for plans of up to
// two rows, else 4) are loaded together with the tile's k inputs, so the
// pipelined form has them in flight one tile ahead, like the inputs, and the
// in-order load counter never makes a compare wait for a load issued after
// the next tile's.  Plans with more rows than R take the further rows in
// blocks of R, loaded just before their math.
//
// Accounting: the clean case costs an xor/or reduction, one compare and one
// wave-uniform branch per row per tile -- no atomics, no stores.  On the rare
// path (some lane differs) the tile's count and lowest column are found with
// ballots and folded into per-wave running values: lane i carries row i's
// count and first column (three VGPRs, no LDS; a launch covers at most 64
// rows, plans with more are launched in row blocks of 64).  A wave flushes once
// per object segment, one atomicAdd and one atomicMin (unsigned long long) per
// row whose count is non-zero, so the atomics of a launch are bounded by
// waves x segments x rows whatever the data.
//
// Forms: rs_verify_pipe_kernel (shards under 4 GiB: wave-uniform 64-bit bases
// plus 32-bit lane offsets, next tile's loads issued before this tile's math),
// rs_verify_kernel (64-bit offsets: larger shards and slime_rs_kernel_pipeline(0)),
// rs_verify_bytes_kernel (object slots: big-endian words XOR mapping[o]) and
// rs_verify_column_kernel (one column per lane: generic k through wide_dot,
// and layouts that are not 4-byte aligned).  Wide codes (k > 16) are correct
// through the column form; a matrix-core verify is out of scope.  The schedule
// is the static one with column segments (object_segments).
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "rs_apply_kernel.hpp"
#include "rs_ragged_launch.hpp"  // with_k
#include "rs_verify_kernel.hpp"  // Tally, load_tile, check_tile, check_columns: shared with rs_verify_ragged.hip

namespace slime {
namespace verify {

// Strides are in BYTES in every kernel here (the symbol entry point scales
// its uint32 strides): one body serves symbols and object slots.
#define SLIME_VERIFY_PARAMS                                                                                        \
  const uint8_t *__restrict__ in, const uint8_t *__restrict__ cmp, uint64_t in_obj, uint64_t in_shard,             \
      uint64_t cmp_obj, uint64_t cmp_shard, const uint32_t *__restrict__ coeff, const uint32_t *__restrict__ in_idx, \
      const uint32_t *__restrict__ out_idx, const uint32_t *__restrict__ mapping,                                  \
      unsigned long long *__restrict__ mism, unsigned long long *__restrict__ first, uint64_t ncols, uint32_t nobj, \
      uint32_t rows, uint32_t k, uint32_t nseg, uint32_t res_stride

// Software-pipelined vector form: shards under 4 GiB (ncols < 2^30).
template <int K, int U, int R>
__global__ __launch_bounds__(kBlock) void rs_verify_pipe_kernel(SLIME_VERIFY_PARAMS) {
  const uint32_t nvec = (uint32_t)(ncols >> 2);
  const uint32_t seg_vec = apply::segment_vectors(nvec, nseg);
  const uint64_t nwork = (uint64_t)nobj * nseg;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * kWaves;
  Tally t(threadIdx.x & 63);
  for (uint64_t wi = blockIdx.y; wi < nwork; wi += gridDim.y) {
    const uint64_t obj = wi / nseg;
    const uint32_t seg = (uint32_t)(wi % nseg);
    const uint8_t* const ib = in + obj * in_obj;
    const uint8_t* const cb = cmp + obj * cmp_obj;
    t.begin(mism + obj * res_stride, first + obj * res_stride);
    const uint8_t* sb[K];
#pragma unroll
    for (int j = 0; j < K; ++j) sb[j] = ib + (uint64_t)in_idx[j] * in_shard;
    const uint8_t* rb[R];
    row_bases<R>(rb, cb, out_idx, cmp_shard, 0, rows);
    const uint32_t v0 = seg * seg_vec < nvec ? seg * seg_vec : nvec;
    const uint32_t v1 = nvec - v0 > seg_vec ? v0 + seg_vec : nvec;
    const uint32_t ntiles = (v1 - v0 + 64 * U - 1) / (64 * U);
    uint4 xa[U][K], xb[U][K], sa[R][U], sc[R][U];
    uint32_t step = wave;
    if (step < ntiles) load_tile<K, U, R, uint32_t>(xa, sa, sb, rb, v0 + step * (64 * U) + t.lane, v1);
    // The last prefetch of a wave (past ntiles) re-reads its current tile.
    while (step < ntiles) {
      uint32_t next = step + nwaves;
      load_tile<K, U, R, uint32_t>(xb, sc, sb, rb, v0 + (next < ntiles ? next : step) * (64 * U) + t.lane, v1);
      check_tile<K, U, R, false, uint32_t>(t, xa, sa, cb, coeff, out_idx, cmp_shard, rows, 0u, v0 + step * (64 * U), v1);
      step = next;
      if (step >= ntiles) break;
      next = step + nwaves;
      load_tile<K, U, R, uint32_t>(xa, sa, sb, rb, v0 + (next < ntiles ? next : step) * (64 * U) + t.lane, v1);
      check_tile<K, U, R, false, uint32_t>(t, xb, sc, cb, coeff, out_idx, cmp_shard, rows, 0u, v0 + step * (64 * U), v1);
      step = next;
    }
    // Columns past the last whole vector (at most three): one wave of the
    // object's last segment.
    if (seg == nseg - 1 && wave == 0 && (ncols & 3))
      check_columns<K, false>(t, ib, cb, coeff, in_idx, in_shard, out_idx, cmp_shard, rows, k, 0u,
                              (uint64_t)nvec << 2, ncols);
    t.flush();
  }
}

// Vector form with 64-bit offsets (any shard size); BYTES: object slots.
template <int K, int U, int R, bool BYTES>
__device__ __forceinline__ void verify_body(SLIME_VERIFY_PARAMS) {
  const uint64_t nvec = ncols >> 2;
  const uint64_t seg_vec = apply::segment_vectors(nvec, nseg);
  const uint64_t nwork = (uint64_t)nobj * nseg;
  const uint64_t wave = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
  Tally t(threadIdx.x & 63);
  for (uint64_t wi = blockIdx.y; wi < nwork; wi += gridDim.y) {
    const uint64_t obj = wi / nseg, seg = wi % nseg;
    const uint8_t* const ib = in + obj * in_obj;
    const uint8_t* const cb = cmp + obj * cmp_obj;
    uint32_t m = 0;
    if constexpr (BYTES) m = mapping[obj];
    t.begin(mism + obj * res_stride, first + obj * res_stride);
    const uint8_t* sb[K];
#pragma unroll
    for (int j = 0; j < K; ++j) sb[j] = ib + (uint64_t)in_idx[j] * in_shard;
    const uint8_t* rb[R];
    row_bases<R>(rb, cb, out_idx, cmp_shard, 0, rows);
    const uint64_t v0 = seg * seg_vec < nvec ? seg * seg_vec : nvec;
    const uint64_t v1 = v0 + seg_vec < nvec ? v0 + seg_vec : nvec;
    const uint64_t ntiles = (v1 - v0 + 64 * U - 1) / (64 * U);
    for (uint64_t step = wave; step < ntiles; step += nwaves) {
      const uint64_t tb = v0 + step * (64 * U);
      uint4 x[U][K], s[R][U];
      load_tile<K, U, R, uint64_t>(x, s, sb, rb, tb + t.lane, v1);
      check_tile<K, U, R, BYTES, uint64_t>(t, x, s, cb, coeff, out_idx, cmp_shard, rows, m, tb, v1);
    }
    if (seg == nseg - 1 && wave == 0 && (ncols & 3))
      check_columns<K, BYTES>(t, ib, cb, coeff, in_idx, in_shard, out_idx, cmp_shard, rows, k, m, nvec << 2, ncols);
    t.flush();
  }
}

template <int K, int U, int R>
__global__ __launch_bounds__(kBlock) void rs_verify_kernel(SLIME_VERIFY_PARAMS) {
  verify_body<K, U, R, false>(in, cmp, in_obj, in_shard, cmp_obj, cmp_shard, coeff, in_idx, out_idx, mapping, mism,
                              first, ncols, nobj, rows, k, nseg, res_stride);
}

// Object slots: slot o at in + o*in_obj, chunk c at slot + c*in_shard (cmp is
// the same base); words are big-endian bytes XOR mapping[o], and a column
// mismatches iff BE(stored) != computed ^ mapping[o].
template <int K, int U, int R>
__global__ __launch_bounds__(kBlock) void rs_verify_bytes_kernel(SLIME_VERIFY_PARAMS) {
  verify_body<K, U, R, true>(in, cmp, in_obj, in_shard, cmp_obj, cmp_shard, coeff, in_idx, out_idx, mapping, mism,
                             first, ncols, nobj, rows, k, nseg, res_stride);
}

// Column form: every column one per lane, generic k (nseg is 1).
template <bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_verify_column_kernel(SLIME_VERIFY_PARAMS) {
  Tally t(threadIdx.x & 63);
  const uint64_t w0 = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u);
  const uint64_t nthr = (uint64_t)gridDim.x * kBlock;
  for (uint64_t obj = blockIdx.y; obj < nobj; obj += gridDim.y) {
    uint32_t m = 0;
    if constexpr (BYTES) m = mapping[obj];
    t.begin(mism + obj * res_stride, first + obj * res_stride);
    for (uint64_t bw = w0; bw < ncols; bw += nthr)
      check_columns<0, BYTES>(t, in + obj * in_obj, cmp + obj * cmp_obj, coeff, in_idx, in_shard, out_idx, cmp_shard,
                              rows, k, m, bw, ncols);
    t.flush();
  }
}

#undef SLIME_VERIFY_PARAMS

// The result arrays' initial state: no mismatches, no first column.  It runs
// ahead of the verify kernels on the same stream, so every launch -- and
// every replay of a graph that captured one -- starts from it.  A kernel node,
// so a captured verify is kernel nodes only (DESIGN.md §14 on memset nodes).
__global__ __launch_bounds__(kBlock) void rs_verify_init_kernel(unsigned long long* __restrict__ mism,
                                                                unsigned long long* __restrict__ first,
                                                                uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    mism[i] = 0;
    first[i] = ~0ull;
  }
}

}  // namespace verify

namespace {

using apply::kBlock;

// 16-byte units per lane per tile: the tile's K inputs and R stored rows for
// U units are held at once (twice in the pipelined form), about 24 vectors.
constexpr int verify_unroll_c(int K, int R) {
  return 24 / (K + R) > 4 ? 4 : 24 / (K + R) < 1 ? 1 : 24 / (K + R);
}

#define SLIME_VERIFY_ARGS(v, rows_c, r0)                                                                           \
  (const uint8_t*)(v).in, (const uint8_t*)(v).cmp, (v).in_obj_stride, (v).in_shard_stride, (v).cmp_obj_stride,     \
      (v).cmp_shard_stride, (v).coeff + (uint64_t)(r0) * coeff_stride((v).k), (v).in_idx, (v).out_idx + (r0),      \
      (v).mapping, (unsigned long long*)(v).mismatches + (r0), (unsigned long long*)(v).first + (r0), (v).ncols,   \
      (v).nobj, (rows_c), (v).k

dim3 vector_grid(const VerifyLaunch& v, uint32_t nseg, uint64_t target, int U) {
  const uint64_t nwork = (uint64_t)v.nobj * nseg;
  const uint64_t gy = nwork < 65535 ? nwork : 65535;
  const uint64_t per_block = 4ull * kBlock * U;
  uint64_t gx = (target + gy - 1) / gy;
  const uint64_t need = (v.ncols / nseg + per_block - 1) / per_block;
  if (gx > need) gx = need;
  if (gx < 1) gx = 1;
  return dim3((uint32_t)gx, (uint32_t)gy);
}

// The pipelined kernel's 32-bit byte offsets need shards under 4 GiB.
bool pipe_ok(const VerifyLaunch& v) { return !v.bytes && pipelined_kernels() && v.ncols < (1ull << 30); }

template <int K, int R>
hipError_t launch_vec(const VerifyLaunch& v, uint32_t r0, uint32_t rows_c, hipStream_t s) {
  constexpr int U = verify_unroll_c(K, R);
  const uint32_t nseg = object_segments(v.nobj, v.ncols);
  if (v.bytes) {
    hipLaunchKernelGGL((verify::rs_verify_bytes_kernel<K, U, R>), vector_grid(v, nseg, 512, U), dim3(kBlock), 0, s,
                       SLIME_VERIFY_ARGS(v, rows_c, r0), nseg, v.rows);
  } else if (pipe_ok(v)) {
    // Fat waves, one block a CU; thin ones (U = 1) four, as the apply launch.
    hipLaunchKernelGGL((verify::rs_verify_pipe_kernel<K, U, R>), vector_grid(v, nseg, U == 1 ? 1024 : 256, U),
                       dim3(kBlock), 0, s, SLIME_VERIFY_ARGS(v, rows_c, r0), nseg, v.rows);
  } else {
    hipLaunchKernelGGL((verify::rs_verify_kernel<K, U, R>), vector_grid(v, nseg, 512, U), dim3(kBlock), 0, s,
                       SLIME_VERIFY_ARGS(v, rows_c, r0), nseg, v.rows);
  }
  return hipGetLastError();
}

template <int K>
hipError_t launch_rows(const VerifyLaunch& v, uint32_t r0, uint32_t rows_c, hipStream_t s) {
  return rows_c <= 2 ? launch_vec<K, 2>(v, r0, rows_c, s) : launch_vec<K, 4>(v, r0, rows_c, s);
}

hipError_t launch_columns(const VerifyLaunch& v, uint32_t r0, uint32_t rows_c, hipStream_t s) {
  const uint64_t gy = v.nobj < 65535 ? v.nobj : 65535;
  uint64_t gx = (512 + gy - 1) / gy;
  const uint64_t need = (v.ncols + kBlock - 1) / kBlock;
  if (gx > need) gx = need;
  if (gx < 1) gx = 1;
  const dim3 grid((uint32_t)gx, (uint32_t)gy);
  if (v.bytes)
    hipLaunchKernelGGL((verify::rs_verify_column_kernel<true>), grid, dim3(kBlock), 0, s,
                       SLIME_VERIFY_ARGS(v, rows_c, r0), 1u, v.rows);
  else
    hipLaunchKernelGGL((verify::rs_verify_column_kernel<false>), grid, dim3(kBlock), 0, s,
                       SLIME_VERIFY_ARGS(v, rows_c, r0), 1u, v.rows);
  return hipGetLastError();
}

hipError_t launch_block(const VerifyLaunch& v, uint32_t r0, uint32_t rows_c, hipStream_t s) {
  if (!v.vec_ok || v.k < 1 || v.k > 16) return launch_columns(v, r0, rows_c, s);
  return ragged::with_k(v.k, [&](auto kc) { return launch_rows<decltype(kc)::value>(v, r0, rows_c, s); });
}

#undef SLIME_VERIFY_ARGS

}  // namespace

hipError_t launch_verify_init(uint64_t* mismatches, uint64_t* first, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(verify::rs_verify_init_kernel, dim3((uint32_t)(blocks < 1024 ? blocks : 1024)), dim3(kBlock), 0,
                     s, (unsigned long long*)mismatches, (unsigned long long*)first, n);
  return hipGetLastError();
}

hipError_t launch_verify(const VerifyLaunch& v, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (v.nobj == 0 || v.rows == 0) return hipSuccess;
  if (hipError_t e = launch_verify_init(v.mismatches, v.first, (uint64_t)v.nobj * v.rows, s)) return e;
  if (v.ncols == 0) return hipSuccess;
  // A launch tallies at most 64 rows (one lane each): larger plans go in row blocks.
  for (uint32_t r0 = 0; r0 < v.rows; r0 += 64) {
    const uint32_t rows_c = v.rows - r0 < 64 ? v.rows - r0 : 64;
    if (hipError_t e = launch_block(v, r0, rows_c, s)) return e;
  }
  return hipSuccess;
}

}  // namespace slime
