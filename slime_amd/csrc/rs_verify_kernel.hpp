// The compare of the device-side verify, shared by the uniform kernels
// (rs_verify.hip) and the ragged ones (rs_verify_ragged.hip): a wave's running
// mismatch record (Tally), a tile's loads (load_tile: k inputs and R stored
// rows for U 16-byte units a lane), the compare of a loaded tile against a
// plan's rows (check_tile) and the one-column-per-lane form (check_columns).
// What differs between the two files is only where a wave's tiles come from.
// rs_verify.hip's header comment describes the scheme.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

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

}  // namespace verify
}  // namespace slime
