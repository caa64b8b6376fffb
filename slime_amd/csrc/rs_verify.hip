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

#include <type_traits>

#include "kernels.hpp"
#include "rs_apply_kernel.hpp"

namespace slime {
namespace verify {

using apply::CoeffRow;
using apply::kBlock;
using apply::kWaves;
using apply::load_coeff_row;

__device__ __forceinline__ uint32_t be(uint32_t w) { return __builtin_bswap32(w); }

// A wave's running mismatch record: lane i holds row i's count and lowest
// column since the last flush.
struct Tally {
  uint32_t lane;
  uint32_t cnt = 0;
  uint64_t first = ~0ull;
  unsigned long long* mism = nullptr;  // the current object's result rows
  unsigned long long* fst = nullptr;
  __device__ __forceinline__ explicit Tally(uint32_t lane_) : lane(lane_) {}
  __device__ __forceinline__ void begin(unsigned long long* m, unsigned long long* f) {
    mism = m;
    fst = f;
  }
  // Once per (wave, object segment); also whenever a count could wrap.
  __device__ __forceinline__ void flush() {
    if (cnt != 0) {  // only lanes below `rows` ever count
      atomicAdd(mism + lane, (unsigned long long)cnt);
      atomicMin(fst + lane, (unsigned long long)first);
    }
    cnt = 0;
    first = ~0ull;
  }
  // Rare path: n (<= 1024) mismatching columns of `row`, the lowest at col;
  // all three wave-uniform.
  __device__ __forceinline__ void add(uint32_t row, uint32_t n, uint64_t col) {
    if (lane == row) {
      cnt += n;
      first = col < first ? col : first;
    }
    if (__ballot(cnt >= 0x80000000u)) flush();
  }
};

// 16-byte load of vector g of a shard: 32-bit byte offset off a wave-uniform
// base (T = uint32_t, shards under 4 GiB) or a 64-bit address.
template <class T>
__device__ __forceinline__ uint4 ldv(const uint8_t* base, T g) {
  if constexpr (std::is_same<T, uint32_t>::value)
    return apply::ld16_at<true>(reinterpret_cast<const uint32_t*>(base), g << 4);
  else
    return apply::ld16<true>(reinterpret_cast<const uint32_t*>(base + (g << 4)));
}

// A tile's loads: k inputs and R stored rows for U units, all unconditional
// (lanes past the segment end re-read its last vector), so the waitcnt pass
// sees a fixed count per tile.
template <int K, int U, int R, class T>
__device__ __forceinline__ void load_tile(uint4 (&x)[U][K], uint4 (&s)[R][U], const uint8_t* const (&sb)[K],
                                          const uint8_t* const (&rb)[R], T g0, T v1) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const T g = g0 + 64 * u < v1 ? g0 + 64 * u : v1 - 1;
#pragma unroll
    for (int j = 0; j < K; ++j) x[u][j] = ldv<T>(sb[j], g);
  }
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const T g = g0 + 64 * u < v1 ? g0 + 64 * u : v1 - 1;
      s[i][u] = ldv<T>(rb[i], g);
    }
  // The scheduler may not sink these loads into the math that follows: left
  // alone it issued the next tile's loads after the current tile's first row.
  __builtin_amdgcn_sched_barrier(0);
}

// Stored-row bases of row block r0 (rows past the plan's last re-read it).
template <int R>
__device__ __forceinline__ void row_bases(const uint8_t* (&rb)[R], const uint8_t* cb,
                                          const uint32_t* __restrict__ out_idx, uint64_t cmp_shard, uint32_t r0,
                                          uint32_t rows) {
#pragma unroll
  for (int i = 0; i < R; ++i) rb[i] = cb + (uint64_t)out_idx[r0 + i < rows ? r0 + i : rows - 1] * cmp_shard;
}

// Bits of the words that differ between a computed and a stored vector.
template <bool BYTES>
__device__ __forceinline__ uint4 delta4(uint4 r, uint4 s, uint32_t m) {
  if constexpr (BYTES) r = make_uint4(be(r.x ^ m), be(r.y ^ m), be(r.z ^ m), be(r.w ^ m));
  return make_uint4(r.x ^ s.x, r.y ^ s.y, r.z ^ s.z, r.w ^ s.w);
}

// Rare path of one row of a tile: count and lowest column by ballots.
template <int U, bool BYTES>
__device__ __forceinline__ void tally_row(Tally& t, uint32_t row, const uint4 (&r)[U], const uint4 (&s)[U],
                                          const bool (&ok)[U], uint32_t m, uint64_t tb) {
  uint32_t n = 0;
  uint64_t col = ~0ull;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint4 e = delta4<BYTES>(r[u], s[u], m);
    const uint32_t d = ok[u] ? (e.x ? 1u : 0u) | (e.y ? 2u : 0u) | (e.z ? 4u : 0u) | (e.w ? 8u : 0u) : 0u;
    n += __popcll(__ballot(d & 1u)) + __popcll(__ballot(d & 2u)) + __popcll(__ballot(d & 4u)) +
         __popcll(__ballot(d & 8u));
    const uint64_t any = __ballot(d != 0);
    if (any && col == ~0ull) {  // units, lanes and words are all in column order
      const uint32_t l = (uint32_t)__ffsll((unsigned long long)any) - 1;
      const uint32_t dl = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)l);
      col = ((tb + 64 * u + l) << 2) + ((uint32_t)__ffs((int)dl) - 1);
    }
  }
  t.add(row, n, col);
}

// Rows [r0, r0 + R) of a tile against the stored rows in s.  Row r0 always
// exists and reads every input of the tile (see rs_apply_pipe_kernel: the
// waitcnt pass resolves the tile's loads there).
template <int K, int U, int R, bool BYTES>
__device__ __forceinline__ void check_rows(Tally& t, const uint4 (&x)[U][K], const uint4 (&s)[R][U],
                                           const bool (&ok)[U], const uint32_t* __restrict__ coeff, uint32_t r0,
                                           uint32_t rows, uint32_t m, uint64_t tb) {
#pragma unroll
  for (int i = 0; i < R; ++i) {
    if (i == 0 || r0 + i < rows) {
      const CoeffRow<K> c = load_coeff_row<K>(coeff, r0 + i);
      uint4 r[U];
      uint32_t any = 0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        r[u] = apply::dot4<K>(x[u], c);
        const uint4 e = delta4<BYTES>(r[u], s[i][u], m);
        any |= ok[u] ? e.x | e.y | e.z | e.w : 0u;
      }
      if (__ballot(any != 0)) tally_row<U, BYTES>(t, r0 + i, r, s[i], ok, m, tb);
    }
  }
}

// One tile: vectors [tb, tb + 64 U) clipped to v1, inputs x and the first R
// stored rows s already loaded.
template <int K, int U, int R, bool BYTES, class T>
__device__ __forceinline__ void check_tile(Tally& t, uint4 (&x)[U][K], uint4 (&s)[R][U], const uint8_t* cb,
                                           const uint32_t* __restrict__ coeff,
                                           const uint32_t* __restrict__ out_idx, uint64_t cmp_shard, uint32_t rows,
                                           uint32_t m, T tb, T v1) {
  bool ok[U];
#pragma unroll
  for (int u = 0; u < U; ++u) ok[u] = tb + 64 * u + t.lane < v1;
  if constexpr (BYTES) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < K; ++j)
        x[u][j] = make_uint4(be(x[u][j].x) ^ m, be(x[u][j].y) ^ m, be(x[u][j].z) ^ m, be(x[u][j].w) ^ m);
  }
  check_rows<K, U, R, BYTES>(t, x, s, ok, coeff, 0, rows, m, (uint64_t)tb);
  // Plans of more than R rows: the further row blocks, loaded here.
  for (uint32_t r0 = R; r0 < rows; r0 += R) {
    const uint8_t* rb[R];
    row_bases<R>(rb, cb, out_idx, cmp_shard, r0, rows);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const T g = tb + 64 * u + t.lane < v1 ? tb + 64 * u + t.lane : v1 - 1;
        s[i][u] = ldv<T>(rb[i], g);
      }
    check_rows<K, U, R, BYTES>(t, x, s, ok, coeff, r0, rows, m, (uint64_t)tb);
  }
}

// One column per lane: column bw + lane of the object at ib / cb, every row.
// bw is the wave's first column (always inside the object); lanes past the
// last column re-read column bw and never count.  K > 0: compile-time k, the
// inputs held in registers; K == 0: generic k through wide_dot.
template <int K, bool BYTES>
__device__ __forceinline__ void check_columns(Tally& t, const uint8_t* ib, const uint8_t* cb,
                                              const uint32_t* __restrict__ coeff,
                                              const uint32_t* __restrict__ in_idx, uint64_t in_shard,
                                              const uint32_t* __restrict__ out_idx, uint64_t cmp_shard,
                                              uint32_t rows, uint32_t k, uint32_t m, uint64_t bw, uint64_t ncols) {
  const bool ok = bw + t.lane < ncols;
  const uint64_t off = (ok ? bw + t.lane : bw) << 2;
  auto in_word = [&](uint32_t j) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(ib + (uint64_t)in_idx[j] * in_shard + off);
    return BYTES ? be(w) ^ m : w;
  };
  uint32_t x[K > 0 ? K : 1];
  if constexpr (K > 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) x[j] = in_word(j);
  }
  for (uint32_t i = 0; i < rows; ++i) {
    uint32_t r;
    if constexpr (K > 0) {
      const CoeffRow<K> c = load_coeff_row<K>(coeff, i);
      uint64_t lo = 0;
      uint32_t hi = 0;
#pragma unroll
      for (int j = 0; j < K; ++j) mac(lo, hi, x[j], c[j]);
      r = fold96(lo, hi);
    } else {
      r = apply::wide_dot(coeff + (uint64_t)i * apply::wide_coeff_stride(k), k, in_word);
    }
    const uint32_t stored = *reinterpret_cast<const uint32_t*>(cb + (uint64_t)out_idx[i] * cmp_shard + off);
    const uint64_t bad = __ballot(ok && stored != (BYTES ? be(r ^ m) : r));
    if (bad) t.add(i, (uint32_t)__popcll(bad), bw + (uint32_t)__ffsll((unsigned long long)bad) - 1);
  }
}

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
  if (!v.vec_ok) return launch_columns(v, r0, rows_c, s);
  switch (v.k) {
    case 1: return launch_rows<1>(v, r0, rows_c, s);
    case 2: return launch_rows<2>(v, r0, rows_c, s);
    case 3: return launch_rows<3>(v, r0, rows_c, s);
    case 4: return launch_rows<4>(v, r0, rows_c, s);
    case 5: return launch_rows<5>(v, r0, rows_c, s);
    case 6: return launch_rows<6>(v, r0, rows_c, s);
    case 7: return launch_rows<7>(v, r0, rows_c, s);
    case 8: return launch_rows<8>(v, r0, rows_c, s);
    case 9: return launch_rows<9>(v, r0, rows_c, s);
    case 10: return launch_rows<10>(v, r0, rows_c, s);
    case 11: return launch_rows<11>(v, r0, rows_c, s);
    case 12: return launch_rows<12>(v, r0, rows_c, s);
    case 13: return launch_rows<13>(v, r0, rows_c, s);
    case 14: return launch_rows<14>(v, r0, rows_c, s);
    case 15: return launch_rows<15>(v, r0, rows_c, s);
    case 16: return launch_rows<16>(v, r0, rows_c, s);
    default: return launch_columns(v, r0, rows_c, s);
  }
}

#undef SLIME_VERIFY_ARGS

}  // namespace

hipError_t launch_verify(const VerifyLaunch& v, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (v.nobj == 0 || v.rows == 0) return hipSuccess;
  const uint64_t n = (uint64_t)v.nobj * v.rows;
  const uint64_t blocks = (n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(verify::rs_verify_init_kernel, dim3((uint32_t)(blocks < 1024 ? blocks : 1024)), dim3(kBlock), 0,
                     s, (unsigned long long*)v.mismatches, (unsigned long long*)v.first, n);
  if (hipError_t e = hipGetLastError()) return e;
  if (v.ncols == 0) return hipSuccess;
  // A launch tallies at most 64 rows (one lane each): larger plans go in row blocks.
  for (uint32_t r0 = 0; r0 < v.rows; r0 += 64) {
    const uint32_t rows_c = v.rows - r0 < 64 ? v.rows - r0 : 64;
    if (hipError_t e = launch_block(v, r0, rows_c, s)) return e;
  }
  return hipSuccess;
}

}  // namespace slime
