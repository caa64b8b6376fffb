// Device side of the pair locate (rs_locate_pairs_ragged.hip): the bodies of
// rs_locate_ragged_kernel.hpp again, over its helpers (filtered_out, flag_tile,
// tally_slots) and with the same fast path, with the pair rule of
// locate_rule.hpp on the rare path.  They are bodies of their own, not the
// one-shard bodies behind a compile-time flag: the one-shard kernels' machine
// code is compared byte for byte from commit to commit (tools/kernel_ids.py),
// and a flag through the shared bodies moved the bytes of eight of them.
//
// What differs from the one-shard bodies: a flagged column goes through
// classify_pair_column, which leaves the column's syndromes in the lane's slice
// of the block's LDS strip and may name two slots; tally_slots then runs once
// per named slot, and a tail item issues its atomics for both.
#pragma once
#include <hip/hip_runtime.h>

#include "rs_locate_ragged_kernel.hpp"

namespace slime {
namespace locate {

// The pair rule's classification of one column (locate_rule.hpp, pair_slots): classify_column's
// pass, which also writes the column's syndromes into the lane's slice of the block's LDS strip --
// `strip` is rows x kBlock words, s_i at strip[i * kBlock + threadIdx.x], so a wave's accesses to
// one row fall into 64 consecutive words -- and keeps the d_i in a register mask.  A column the
// one-shard rule leaves unlocated then goes through the pair enumeration, which reads the strip
// and the plan's coefficient rows.  No per-row arrays in registers, nothing in scratch.
template <bool BYTES>
__device__ __forceinline__ Slots classify_pair_column(const uint8_t* ib, const uint8_t* cb,
                                                      const uint32_t* __restrict__ coeff,
                                                      const uint32_t* __restrict__ in_idx, uint64_t in_shard,
                                                      const uint32_t* __restrict__ out_idx, uint64_t cmp_shard,
                                                      uint32_t rows, uint32_t k, uint32_t m, uint64_t col,
                                                      uint32_t* strip) {
  const uint32_t cs = apply::wide_coeff_stride(k);
  auto in_word = [&](uint32_t j) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(ib + (uint64_t)in_idx[j] * in_shard + (col << 2));
    return BYTES ? be(v) ^ m : v;
  };
  uint32_t* const mine = strip + threadIdx.x;
  Column c;
  c.begin(k);
  uint64_t dmask = 0;
  for (uint32_t i = 0; i < rows; ++i) {
    const uint32_t* const ci = coeff + (uint64_t)i * cs;
    const uint32_t computed = apply::wide_dot(ci, k, in_word);
    const uint32_t w = *reinterpret_cast<const uint32_t*>(cb + (uint64_t)out_idx[i] * cmp_shard + (col << 2));
    const uint32_t stored = BYTES ? be(w) ^ m : w;
    c.row(i, computed, stored, coeff, ci);
    dmask |= (uint64_t)(stored != computed) << i;
    mine[i * kBlock] = sub(canon(stored), computed);
  }
  return pair_slots(
      c.slot(k, rows), dmask, [&](uint32_t i) { return mine[i * kBlock]; },
      [&](uint32_t i, uint32_t j) { return coeff[(uint64_t)i * cs + j]; }, k, rows);
}

// The tail items: one {object, column} per lane, classified and counted by the lane itself, for
// both slots of a pair.
template <bool SET, bool BYTES>
__device__ __forceinline__ void locate_pairs_tails(SLIME_RLOCATE_PARAMS, uint32_t* strip) {
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t nthr = (uint64_t)gridDim.x * kBlock;
  const uint32_t nslots = k + rows + 1;
  for (uint64_t t = tid; t < ntails; t += nthr) {
    const Tail it = tails[t];
    if (filtered_out(filter, it.obj, rows)) continue;
    const Desc* const d = descs + it.obj;
    PlanRows pl{coeff, out_idx, rows};
    const uint32_t* iidx = in_idx;
    if constexpr (SET) {
      const PlanRef p = ragged::read_plan(coeff, d);
      pl = ragged::whole_plan(coeff, p);
      iidx = coeff + p.in_off;
    }
    uint32_t m = 0;
    if constexpr (BYTES) m = mapping[it.obj];
    Slots ps =
        classify_pair_column<BYTES>(in + (d->src_off << 2), cmp + (d->dst_off << 2), pl.coeff, iidx,
                                    d->src_shard << 2, pl.oidx, d->dst_shard << 2, pl.rows, k, m, it.col, strip);
    if constexpr (SET) ps = set_slots(ps, k, pl.rows, rows);
    if (ps.a != kNoSlot) {
      atomicAdd(counts + (uint64_t)it.obj * nslots + ps.a, 1ull);
      atomicMin(first + (uint64_t)it.obj * nslots + ps.a, (unsigned long long)it.col);
    }
    if (ps.b != kNoSlot) {  // a pair: the column counts for both of its slots
      atomicAdd(counts + (uint64_t)it.obj * nslots + ps.b, 1ull);
      atomicMin(first + (uint64_t)it.obj * nslots + ps.b, (unsigned long long)it.col);
    }
  }
}

// Four columns a lane, k = K <= 16 over 4-byte aligned bases: locate_vectors with four stored rows
// a step (pair launches have rows >= 4) and the pair rule on the rare path.
template <int K, int W, int UB, int C, bool SET, bool BYTES>
__device__ __forceinline__ void locate_pairs_vectors(SLIME_RLOCATE_PARAMS, uint32_t* strip) {
  static_assert(K > 0 && K <= 16 && W >= 1 && W <= UB && W <= 4, "compile-time k; a step is at most a tile");
  constexpr int R = 4;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nslots = k + rows + 1;
  UnitWalk<C, 1, false> w(nullptr, units, descs, nunits, lane, wave, gridDim.x * kWaves);
  Tally t(lane);
  const uint8_t* sb[K];
  const uint8_t* rb[R];
#pragma unroll
  for (int j = 0; j < K; ++j) sb[j] = in;
#pragma unroll
  for (int i = 0; i < R; ++i) rb[i] = cmp;
  const uint8_t* ib = in;
  const uint8_t* cb = cmp;
  uint64_t ishard = 0, cshard = 0;
  uint32_t m = 0;
  // The current object's plan and its input indices: the launch's, or with SET placeholders inside
  // the table until the walk enters an object.
  PlanRows pl{coeff, SET ? coeff : out_idx, SET ? 1 : rows};
  const uint32_t* iidx = SET ? coeff : in_idx;
  bool skip = false;
  while (w.live) {
    if (w.fresh) {  // the first tile since the object changed
      skip = filtered_out(filter, w.obj, rows);
      if (!skip) {
        if constexpr (BYTES) m = mapping[w.obj];  // wave-uniform
        ib = in + (w.d.src_off << 2);
        ishard = w.d.src_shard << 2;
        if constexpr (SET) {
          const PlanRef p = ragged::load_plan(coeff, descs, w.obj);
          pl = ragged::whole_plan(coeff, p);
          iidx = coeff + p.in_off;
          const u32x16 idx = *reinterpret_cast<const u32x16*>(iidx);  // K <= 16: one line of the table
#pragma unroll
          for (int j = 0; j < K; ++j) sb[j] = ib + (uint64_t)idx[j] * ishard;
        } else {
#pragma unroll
          for (int j = 0; j < K; ++j) sb[j] = ib + (uint64_t)in_idx[j] * ishard;
        }
        cb = cmp + (w.d.dst_off << 2);
        cshard = w.d.dst_shard << 2;
        verify::row_bases<R>(rb, cb, pl.oidx, cshard, 0, pl.rows);
        unsigned long long* const res = counts + (uint64_t)w.obj * nslots;
        if (res != t.mism) {
          t.flush();
          t.begin(res, first + (uint64_t)w.obj * nslots);
        }
      }
    }
    if (!skip) {
      const uint32_t t0 = w.tile() * (64 * UB);
      const uint32_t tend = w.d.nvec - t0 < 64u * UB ? w.d.nvec : t0 + 64 * UB;  // the host lists tiles below nvec
      for (uint32_t tb = t0; tb < tend; tb += 64 * W) {
        uint4 x[W][K], s[R][W];
        verify::load_tile<K, W, R, uint32_t>(x, s, sb, rb, tb + lane, tend);
        const uint32_t bits =
            flag_tile<K, W, R, BYTES, uint32_t>(x, s, cb, pl.coeff, pl.oidx, cshard, pl.rows, m, tb, tend, lane);
        if (__ballot(bits != 0)) {
          // Rare path: word q & 3 of unit q >> 2, every lane that flagged it; for one q the lanes
          // are in column order, for a pair's first slots and for its second slots alike.
          for (uint32_t q = 0; q < 4u * W; ++q) {
            const bool hit = (bits >> q) & 1u;
            if (!__ballot(hit)) continue;
            const uint64_t col = ((uint64_t)(tb + 64 * (q >> 2) + lane) << 2) + (q & 3u);
            Slots ps{kNoSlot, kNoSlot};
            if (hit) {
              ps = classify_pair_column<BYTES>(ib, cb, pl.coeff, iidx, ishard, pl.oidx, cshard, pl.rows, k, m, col,
                                               strip);
              if constexpr (SET) ps = set_slots(ps, k, pl.rows, rows);
            }
            tally_slots(t, ps.a, col);
            tally_slots(t, ps.b, col);
          }
        }
      }
    }
    w.advance();
  }
  t.flush();
  locate_pairs_tails<SET, BYTES>(SLIME_RLOCATE_PASS, strip);
}

// One column a lane over the same unit list: locate_columns with the pair rule on the rare path.
template <bool SET, bool BYTES>
__device__ __forceinline__ void locate_pairs_columns(SLIME_RLOCATE_PARAMS, uint32_t tile_cols, uint32_t unit_tiles,
                                                     uint32_t* strip) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * kWaves;
  const uint32_t nslots = k + rows + 1, cs = apply::wide_coeff_stride(k);
  Tally t(lane);
  for (uint64_t e = wave; e < nunits; e += nwaves) {
    const Unit u = units[e];
    if (filtered_out(filter, u.obj, rows)) continue;
    const ObjRef d = ragged::load_desc(descs, u.obj);
    PlanRows pl{coeff, out_idx, rows};
    const uint32_t* iidx = in_idx;
    if constexpr (SET) {
      const PlanRef p = ragged::load_plan(coeff, descs, u.obj);
      pl = ragged::whole_plan(coeff, p);
      iidx = coeff + p.in_off;
    }
    uint32_t m = 0;
    if constexpr (BYTES) m = mapping[u.obj];
    const uint32_t t1 = d.ntiles - u.tile < unit_tiles ? d.ntiles : u.tile + unit_tiles;
    const uint64_t b0 = (uint64_t)u.tile * tile_cols, bmax = (uint64_t)d.nvec << 2;
    const uint64_t b1 = (uint64_t)t1 * tile_cols < bmax ? (uint64_t)t1 * tile_cols : bmax;
    unsigned long long* const res = counts + (uint64_t)u.obj * nslots;
    if (res != t.mism) {
      t.flush();
      t.begin(res, first + (uint64_t)u.obj * nslots);
    }
    const uint8_t* const ib = in + (d.src_off << 2);
    const uint8_t* const cb = cmp + (d.dst_off << 2);
    const uint64_t ishard = d.src_shard << 2, cshard = d.dst_shard << 2;
    for (uint64_t bw = b0; bw < b1; bw += 64) {
      // bw is always inside the object; lanes past the last column re-read column bw and never count.
      const bool ok = bw + lane < b1;
      const uint64_t col = ok ? bw + lane : bw;
      auto in_word = [&](uint32_t j) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(ib + (uint64_t)iidx[j] * ishard + (col << 2));
        return BYTES ? be(v) ^ m : v;
      };
      bool bad = false;
      for (uint32_t i = 0; i < pl.rows; ++i) {
        const uint32_t r = apply::wide_dot(pl.coeff + (uint64_t)i * cs, k, in_word);
        const uint32_t stored = *reinterpret_cast<const uint32_t*>(cb + (uint64_t)pl.oidx[i] * cshard + (col << 2));
        bad |= stored != (BYTES ? be(r ^ m) : r);
      }
      bad &= ok;
      if (__ballot(bad)) {
        Slots ps{kNoSlot, kNoSlot};
        if (bad) {
          ps = classify_pair_column<BYTES>(ib, cb, pl.coeff, iidx, ishard, pl.oidx, cshard, pl.rows, k, m, col, strip);
          if constexpr (SET) ps = set_slots(ps, k, pl.rows, rows);
        }
        tally_slots(t, ps.a, col);
        tally_slots(t, ps.b, col);
      }
    }
  }
  t.flush();
  locate_pairs_tails<SET, BYTES>(SLIME_RLOCATE_PASS, strip);
}

}  // namespace locate
}  // namespace slime
