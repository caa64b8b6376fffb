// Device side of the ragged verify, symbols (rs_verify_ragged.hip) and stored
// chunk bytes (rs_bytes_ragged.hip, BYTES) alike: what travels with a step,
// the tail items and the one-column-a-lane form; the vector kernel's body is
// rs_verify_ragged_walk_body.hpp.  rs_verify_ragged.hip's header comment
// describes the scheme; the two files hold the __global__ entry points and
// the launches.  BYTES: a stored word is big-endian and XOR-ed with
// its object's mapping value, so inputs are BE(word) ^ m and a column of row i
// mismatches iff the stored word != BE(computed ^ m); `mapping` is read by the
// BYTES forms only.
#pragma once
#include <hip/hip_runtime.h>

#include "planset_table.hpp"
#include "rs_apply_kernel.hpp"
#include "rs_ragged_walk.hpp"
#include "rs_verify_kernel.hpp"
#include "verify_step.hpp"

namespace slime {
namespace verify {

using apply::kCoeffStride;
using apply::u32x16;
using ragged::block_rows;
using ragged::Desc;
using ragged::ObjRef;
using ragged::PlanRef;
using ragged::PlanRows;
using ragged::Tail;
using ragged::Unit;
using ragged::UnitWalk;

// Everything the compare of a step needs, fixed when the step's loads are issued.
struct StepRef {
  const uint8_t* cb;  // the object's stored-row base (bytes) and shard stride
  uint64_t cshard;
  unsigned long long* mism;  // the object's result rows
  unsigned long long* fst;
  PlanRows pl;       // the object's plan
  uint32_t m;        // BYTES: the object's mapping
  uint32_t tb, v1;   // vectors [tb, tb + 64 W) of the object, clipped to v1
};

// coeff: the plan's rows of this row block, or (SET) the set's table; in_idx / out_idx / rows: the
// plan's (unused by SET); r0: the row block (SET); res_stride: the result arrays' row stride.
#define SLIME_RVERIFY_PARAMS                                                                                         \
  const uint8_t *__restrict__ in, const uint8_t *__restrict__ cmp, const Desc *__restrict__ descs,                   \
      const Unit *__restrict__ units, const Tail *__restrict__ tails, const uint32_t *__restrict__ coeff,            \
      const uint32_t *__restrict__ in_idx, const uint32_t *__restrict__ out_idx,                                     \
      const uint32_t *__restrict__ mapping, unsigned long long *__restrict__ mism,                                   \
      unsigned long long *__restrict__ first, uint32_t nunits, uint64_t ntails, uint32_t rows, uint32_t k,           \
      uint32_t r0, uint32_t res_stride
#define SLIME_RVERIFY_PASS \
  in, cmp, descs, units, tails, coeff, in_idx, out_idx, mapping, mism, first, nunits, ntails, rows, k, r0, res_stride

// The tail items: one {object, column} per lane, every row of the block.
// SET: `coeff` is the set's table and the item's plan comes through its
// descriptor.  K == 0: generic k.
template <int K, bool SET, bool BYTES>
__device__ __forceinline__ void verify_tails(SLIME_RVERIFY_PARAMS) {
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t nthr = (uint64_t)gridDim.x * kBlock;
  for (uint64_t t = tid; t < ntails; t += nthr) {
    const Tail it = tails[t];
    const Desc* const d = descs + it.obj;
    const uint32_t* c = coeff;
    const uint32_t* ii = in_idx;
    const uint32_t* oi = out_idx;
    uint32_t nrows = rows;
    if constexpr (SET) {
      const uint32_t* const rec = coeff + (uint64_t)d->reserved[0] * planset::kRecordWords;
      nrows = block_rows(rec[0], r0);
      ii = coeff + rec[1];
      oi = coeff + rec[2] + r0;
      c = coeff + rec[3] + (uint64_t)r0 * apply::wide_coeff_stride(k);
    }
    uint32_t m = 0;
    if constexpr (BYTES) m = mapping[it.obj];
    const uint8_t* const ib = in + ((d->src_off + it.col) << 2);
    const uint8_t* const cb = cmp + ((d->dst_off + it.col) << 2);
    const uint64_t in_shard = d->src_shard << 2, cmp_shard = d->dst_shard << 2;
    auto in_word = [&](uint32_t j) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(ib + (uint64_t)ii[j] * in_shard);
      return BYTES ? be(v) ^ m : v;
    };
    unsigned long long* const mi = mism + (uint64_t)it.obj * res_stride;
    unsigned long long* const f = first + (uint64_t)it.obj * res_stride;
    uint32_t x[K > 0 ? K : 1];
    if constexpr (K > 0) {
#pragma unroll
      for (int j = 0; j < K; ++j) x[j] = in_word(j);
    }
    for (uint32_t i = 0; i < nrows; ++i) {
      uint32_t r;
      if constexpr (K > 0) {
        const CoeffRow<K> cr = load_coeff_row<K>(c, i);
        uint64_t lo = 0;
        uint32_t hi = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) mac(lo, hi, x[j], cr[j]);
        r = fold96(lo, hi);
      } else {
        r = apply::wide_dot(c + (uint64_t)i * apply::wide_coeff_stride(k), k, in_word);
      }
      const uint32_t stored = *reinterpret_cast<const uint32_t*>(cb + (uint64_t)oi[i] * cmp_shard);
      if (stored != (BYTES ? be(r ^ m) : r)) {
        atomicAdd(mi + i, 1ull);
        atomicMin(f + i, (unsigned long long)it.col);
      }
    }
  }
}

// One column per lane over the same unit list (static walk): generic k
// through wide_dot, any alignment.  tile_cols = 256 UB, unit_tiles = C of the
// batch's geometry.
template <bool SET, bool BYTES>
__device__ __forceinline__ void verify_ragged_columns(SLIME_RVERIFY_PARAMS, uint32_t tile_cols, uint32_t unit_tiles) {
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * kWaves;
  Tally t(threadIdx.x & 63);
  for (uint64_t e = wave; e < nunits; e += nwaves) {
    const Unit u = units[e];
    const ObjRef d = ragged::load_desc(descs, u.obj);
    PlanRows pl{coeff, out_idx, rows};
    const uint32_t* ii = in_idx;
    if constexpr (SET) {
      const PlanRef p = ragged::load_plan(coeff, descs, u.obj);
      pl.rows = block_rows(p.rows, r0);
      if (pl.rows == 0) continue;
      pl.coeff = coeff + p.coeff_off + (uint64_t)r0 * apply::wide_coeff_stride(k);
      pl.oidx = coeff + p.out_off + r0;
      ii = coeff + p.in_off;
    }
    uint32_t m = 0;
    if constexpr (BYTES) m = mapping[u.obj];
    const ragged::ColRange c = ragged::unit_columns(d.ntiles, u, tile_cols, unit_tiles, d.nvec);
    unsigned long long* const mi = mism + (uint64_t)u.obj * res_stride;
    if (mi != t.mism) {
      t.flush();
      t.begin(mi, first + (uint64_t)u.obj * res_stride);
    }
    for (uint64_t bw = c.b0; bw < c.b1; bw += 64)
      check_columns<0, BYTES>(t, in + (d.src_off << 2), cmp + (d.dst_off << 2), pl.coeff, ii, d.src_shard << 2, pl.oidx,
                              d.dst_shard << 2, pl.rows, k, m, bw, c.b1);
  }
  t.flush();
  verify_tails<0, SET, BYTES>(SLIME_RVERIFY_PASS);
}

}  // namespace verify
}  // namespace slime
