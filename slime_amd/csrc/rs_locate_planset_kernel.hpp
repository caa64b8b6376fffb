// Device side of the plan-set locate (rs_locate_planset.hip): the ragged
// locate's bodies (rs_locate_ragged_kernel.hpp) with every object classified by
// its OWN plan of a set's table (planset_table.hpp) -- its k input indices, its
// coefficient rows, its output indices and its row count, read when the walk
// enters the object.  The helpers are the single-plan kernels': filtered_out,
// flag_tile, classify_column and tally_slots take the object's plan as their
// arguments; only set_slot (locate_rule.hpp) is added, which puts `unlocated` at
// slot k + max_rows for every object and sends every mismatching column of a
// one-row plan there.  These are separate bodies, not a SET parameter of the
// single-plan ones: those kernels are held to their bytes.
#pragma once
#include <hip/hip_runtime.h>

#include "rs_locate_ragged_kernel.hpp"

namespace slime {
namespace locate {

using apply::u32x16;
using ragged::PlanRef;
using ragged::PlanRows;

// table: the set's; max_rows: its widest plan's rows (the filter's and the results' row stride);
// mapping: BYTES only; filter: NULL or nobj x max_rows counts of a preceding plan-set verify;
// counts / first: nobj x (k + max_rows + 1).
#define SLIME_PLOCATE_PARAMS                                                                                      \
  const uint8_t *__restrict__ in, const uint8_t *__restrict__ cmp, const Desc *__restrict__ descs,                \
      const Unit *__restrict__ units, const Tail *__restrict__ tails, const uint32_t *__restrict__ table,         \
      const uint32_t *__restrict__ mapping, const unsigned long long *__restrict__ filter,                        \
      unsigned long long *__restrict__ counts, unsigned long long *__restrict__ first, uint32_t nunits,           \
      uint64_t ntails, uint32_t max_rows, uint32_t k
#define SLIME_PLOCATE_PASS in, cmp, descs, units, tails, table, mapping, filter, counts, first, nunits, ntails, max_rows, k

// The tail items: one {object, column} per lane, the item's plan read by the lane itself through
// its descriptor (neighbouring lanes hold different objects).
template <bool BYTES>
__device__ __forceinline__ void locate_planset_tails(SLIME_PLOCATE_PARAMS) {
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t nthr = (uint64_t)gridDim.x * kBlock;
  const uint32_t nslots = k + max_rows + 1;
  for (uint64_t t = tid; t < ntails; t += nthr) {
    const Tail it = tails[t];
    if (filtered_out(filter, it.obj, max_rows)) continue;
    const Desc* const d = descs + it.obj;
    const PlanRef p = ragged::read_plan(table, d);
    uint32_t m = 0;
    if constexpr (BYTES) m = mapping[it.obj];
    const uint32_t own = classify_column<BYTES>(in + (d->src_off << 2), cmp + (d->dst_off << 2), table + p.coeff_off,
                                                table + p.in_off, d->src_shard << 2, table + p.out_off,
                                                d->dst_shard << 2, p.rows, k, m, it.col);
    const uint32_t slot = set_slot(own, k, p.rows, max_rows);
    if (slot != kNoSlot) {
      atomicAdd(counts + (uint64_t)it.obj * nslots + slot, 1ull);
      atomicMin(first + (uint64_t)it.obj * nslots + slot, (unsigned long long)it.col);
    }
  }
}

// Four columns a lane, k = K <= 16 over 4-byte aligned bases: locate_ragged_vectors with the
// object's plan taken in the w.fresh block.  R comes from the set's max_rows; row_bases and
// flag_tile clip to the object's own rows.
template <int K, int W, int R, int UB, int C, bool BYTES>
__device__ __forceinline__ void locate_planset_vectors(SLIME_PLOCATE_PARAMS) {
  static_assert(K > 0 && K <= 16 && W >= 1 && W <= UB && W <= 4, "compile-time k; a step is at most a tile");
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nslots = k + max_rows + 1;
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
  PlanRows pl{table, table, 1};     // the current object's plan
  const uint32_t* iidx = table;     // and its input indices
  bool skip = false;
  while (w.live) {
    if (w.fresh) {  // the first tile since the object changed
      skip = filtered_out(filter, w.obj, max_rows);
      if (!skip) {
        const PlanRef p = ragged::load_plan(table, descs, w.obj);
        pl = ragged::whole_plan(table, p);
        iidx = table + p.in_off;
        const u32x16 idx = *reinterpret_cast<const u32x16*>(iidx);  // K <= 16: one line
        if constexpr (BYTES) m = mapping[w.obj];  // wave-uniform
        ib = in + (w.d.src_off << 2);
        ishard = w.d.src_shard << 2;
#pragma unroll
        for (int j = 0; j < K; ++j) sb[j] = ib + (uint64_t)idx[j] * ishard;
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
          // are in column order.
          for (uint32_t q = 0; q < 4u * W; ++q) {
            const bool hit = (bits >> q) & 1u;
            if (!__ballot(hit)) continue;
            const uint64_t col = ((uint64_t)(tb + 64 * (q >> 2) + lane) << 2) + (q & 3u);
            uint32_t slot = kNoSlot;
            if (hit)
              slot = set_slot(classify_column<BYTES>(ib, cb, pl.coeff, iidx, ishard, pl.oidx, cshard, pl.rows, k, m, col),
                              k, pl.rows, max_rows);
            tally_slots(t, slot, col);
          }
        }
      }
    }
    w.advance();
  }
  t.flush();
  locate_planset_tails<BYTES>(SLIME_PLOCATE_PASS);
}

// One column a lane over the same unit list (static walk): generic k through wide_dot, any
// alignment; the unit's object's plan is read per unit.  tile_cols = 256 UB, unit_tiles = C of
// the batch's geometry.
template <bool BYTES>
__device__ __forceinline__ void locate_planset_columns(SLIME_PLOCATE_PARAMS, uint32_t tile_cols, uint32_t unit_tiles) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * kWaves;
  const uint32_t nslots = k + max_rows + 1, cs = apply::wide_coeff_stride(k);
  Tally t(lane);
  for (uint64_t e = wave; e < nunits; e += nwaves) {
    const Unit u = units[e];
    if (filtered_out(filter, u.obj, max_rows)) continue;
    const ObjRef d = ragged::load_desc(descs, u.obj);
    const PlanRef p = ragged::load_plan(table, descs, u.obj);
    const PlanRows pl = ragged::whole_plan(table, p);
    const uint32_t* const iidx = table + p.in_off;
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
        uint32_t slot = kNoSlot;
        if (bad)
          slot = set_slot(classify_column<BYTES>(ib, cb, pl.coeff, iidx, ishard, pl.oidx, cshard, pl.rows, k, m, col), k,
                          pl.rows, max_rows);
        tally_slots(t, slot, col);
      }
    }
  }
  t.flush();
  locate_planset_tails<BYTES>(SLIME_PLOCATE_PASS);
}

}  // namespace locate
}  // namespace slime
