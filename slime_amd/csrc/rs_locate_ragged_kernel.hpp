// Device side of the ragged locate (rs_locate_ragged.hip), symbols and stored
// chunk bytes alike (BYTES: a stored word is big-endian and XOR-ed with its
// object's mapping value, so every symbol is BE(word) ^ m), one plan or a plan
// set's table (SET): the filter's verdict on an object, the fast path's
// per-lane mismatch flags, the rare path's classification of one column by
// locate_rule.hpp, the fold of a wave's classified columns into a Tally (lane =
// slot), the tail items and the one-column-a-lane form.  rs_locate_ragged.hip's
// header comment describes the scheme.
//
// PAIRS: the pair rule of locate_rule.hpp behind the one-shard rule.  A flagged
// column goes through classify_pair_column, which leaves the column's syndromes
// in the lane's slice of the block's LDS strip (`strip`, the bodies' last
// argument; null without PAIRS) and may name two slots; tally_slots then runs
// once per named slot, and a tail item issues its atomics for both.
//
// SET: `coeff` is the set's table (planset_table.hpp) and `rows` its max_rows,
// in_idx / out_idx are null; when the walk enters an object its own plan -- k
// input indices, coefficient rows, output indices, row count -- is read from
// its record, and the column's slot goes through set_slot (locate_rule.hpp).
// The helpers take the object's plan as their arguments either way.
#pragma once
#include <hip/hip_runtime.h>

#include "locate_rule.hpp"
#include "rs_apply_kernel.hpp"
#include "rs_ragged_walk.hpp"
#include "rs_verify_kernel.hpp"

namespace slime {
namespace locate {

using apply::kBlock;
using apply::kWaves;
using apply::u32x16;
using ragged::Desc;
using ragged::ObjRef;
using ragged::PlanRef;
using ragged::PlanRows;
using ragged::Tail;
using ragged::Unit;
using ragged::UnitWalk;
using verify::be;
using verify::Tally;

// coeff / in_idx / out_idx / rows / k: the plan's (SET: the table, null, null, max_rows); mapping:
// BYTES only; filter: NULL or nobj x rows counts of a preceding verify; counts / first: nobj x
// (k + rows + 1).
#define SLIME_RLOCATE_PARAMS                                                                                      \
  const uint8_t *__restrict__ in, const uint8_t *__restrict__ cmp, const Desc *__restrict__ descs,                \
      const Unit *__restrict__ units, const Tail *__restrict__ tails, const uint32_t *__restrict__ coeff,         \
      const uint32_t *__restrict__ in_idx, const uint32_t *__restrict__ out_idx,                                  \
      const uint32_t *__restrict__ mapping, const unsigned long long *__restrict__ filter,                        \
      unsigned long long *__restrict__ counts, unsigned long long *__restrict__ first, uint32_t nunits,           \
      uint64_t ntails, uint32_t rows, uint32_t k
#define SLIME_RLOCATE_PASS \
  in, cmp, descs, units, tails, coeff, in_idx, out_idx, mapping, filter, counts, first, nunits, ntails, rows, k

// true: the filter clears object obj -- all `rows` counts of the verify are zero -- and the launch
// passes over it before any load of its data.
__device__ __forceinline__ bool filtered_out(const unsigned long long* __restrict__ filter, uint32_t obj,
                                             uint32_t rows) {
  if (!filter) return false;
  unsigned long long any = 0;
  for (uint32_t i = 0; i < rows; ++i) any |= filter[(uint64_t)obj * rows + i];
  return any == 0;
}

// The slot of column `col` of the object at ib / cb (bytes; shard strides in bytes), by the rule.
// Re-reads the column's k inputs for every row and its `rows` stored words: the rare path, on
// words the fast path has just loaded.  No per-row arrays.
template <bool BYTES>
__device__ __forceinline__ uint32_t classify_column(const uint8_t* ib, const uint8_t* cb,
                                                    const uint32_t* __restrict__ coeff,
                                                    const uint32_t* __restrict__ in_idx, uint64_t in_shard,
                                                    const uint32_t* __restrict__ out_idx, uint64_t cmp_shard,
                                                    uint32_t rows, uint32_t k, uint32_t m, uint64_t col) {
  const uint32_t cs = apply::wide_coeff_stride(k);
  auto in_word = [&](uint32_t j) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(ib + (uint64_t)in_idx[j] * in_shard + (col << 2));
    return BYTES ? be(v) ^ m : v;
  };
  Column c;
  c.begin(k);
  for (uint32_t i = 0; i < rows; ++i) {
    const uint32_t* const ci = coeff + (uint64_t)i * cs;
    const uint32_t computed = apply::wide_dot(ci, k, in_word);
    const uint32_t w = *reinterpret_cast<const uint32_t*>(cb + (uint64_t)out_idx[i] * cmp_shard + (col << 2));
    c.row(i, computed, BYTES ? be(w) ^ m : w, coeff, ci);
  }
  return c.slot(k, rows);
}

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

// The slots column `col` names under the launch's rule, as either classification above takes its
// arguments; max_rows: the set's, for set_slot.  Without PAIRS .b is kNoSlot.
template <bool PAIRS, bool SET, bool BYTES>
__device__ __forceinline__ Slots column_slots(const uint8_t* ib, const uint8_t* cb,
                                              const uint32_t* __restrict__ coeff,
                                              const uint32_t* __restrict__ in_idx, uint64_t in_shard,
                                              const uint32_t* __restrict__ out_idx, uint64_t cmp_shard,
                                              uint32_t rows, uint32_t k, uint32_t m, uint64_t col, uint32_t max_rows,
                                              uint32_t* strip) {
  if constexpr (PAIRS) {
    Slots ps = classify_pair_column<BYTES>(ib, cb, coeff, in_idx, in_shard, out_idx, cmp_shard, rows, k, m, col, strip);
    if constexpr (SET) ps = set_slots(ps, k, rows, max_rows);
    return ps;
  } else {
    uint32_t slot = classify_column<BYTES>(ib, cb, coeff, in_idx, in_shard, out_idx, cmp_shard, rows, k, m, col);
    if constexpr (SET) slot = set_slot(slot, k, rows, max_rows);
    return Slots{slot, kNoSlot};
  }
}

// Folds a wave's classified columns into its Tally, slot by slot: `slot` is this lane's column's
// slot or kNoSlot, `col` its column; the lanes hold columns in ascending order, so the lowest lane
// of a slot holds its lowest column.
__device__ __forceinline__ void tally_slots(Tally& t, uint32_t slot, uint64_t col) {
  uint64_t left = __ballot(slot != kNoSlot);
  while (left) {
    const int l = __ffsll((unsigned long long)left) - 1;
    const uint32_t sl = (uint32_t)__builtin_amdgcn_readlane((int)slot, l);
    const uint64_t same = __ballot(slot == sl);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)col, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(col >> 32), l);
    t.add(sl, (uint32_t)__popcll(same), ((uint64_t)hi << 32) | lo);
    left &= ~same;
  }
}

// Fast path of one step: vectors [tb, tb + 64 U) clipped to v1, inputs x and the first R stored
// rows s already loaded.  Every row's word deltas are OR-ed per lane across all row blocks;
// returns bit 4u + w set iff word w of unit u has some mismatching row.  No atomics, no stores.
template <int K, int U, int R, bool BYTES, class T>
__device__ __forceinline__ uint32_t flag_tile(uint4 (&x)[U][K], uint4 (&s)[R][U], const uint8_t* cb,
                                              const uint32_t* __restrict__ coeff,
                                              const uint32_t* __restrict__ out_idx, uint64_t cmp_shard,
                                              uint32_t rows, uint32_t m, T tb, T v1, uint32_t lane) {
  if constexpr (BYTES) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < K; ++j)
        x[u][j] = make_uint4(be(x[u][j].x) ^ m, be(x[u][j].y) ^ m, be(x[u][j].z) ^ m, be(x[u][j].w) ^ m);
  }
  uint4 acc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = make_uint4(0, 0, 0, 0);
  auto block = [&](uint32_t r0) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (i == 0 || r0 + i < rows) {
        const apply::CoeffRow<K> c = apply::load_coeff_row<K>(coeff, r0 + i);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint4 e = verify::delta4<BYTES>(apply::dot4<K>(x[u], c), s[i][u], m);
          acc[u] = make_uint4(acc[u].x | e.x, acc[u].y | e.y, acc[u].z | e.z, acc[u].w | e.w);
        }
      }
    }
  };
  block(0);
  // Plans of more than R rows: the further row blocks, loaded here.
  for (uint32_t r0 = R; r0 < rows; r0 += R) {
    const uint8_t* rb[R];
    verify::row_bases<R>(rb, cb, out_idx, cmp_shard, r0, rows);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const T g = tb + 64 * u + lane < v1 ? tb + 64 * u + lane : v1 - 1;
        s[i][u] = verify::ldv<T>(rb[i], g);
      }
    block(r0);
  }
  uint32_t bits = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t d = (acc[u].x ? 1u : 0u) | (acc[u].y ? 2u : 0u) | (acc[u].z ? 4u : 0u) | (acc[u].w ? 8u : 0u);
    if (tb + 64 * u + lane < v1) bits |= d << (4 * u);
  }
  return bits;
}

// The tail items: one {object, column} per lane, classified and counted by the lane itself
// (neighbouring lanes hold different objects: Tally's lane-per-slot scheme does not apply, and
// with SET the lane reads its item's plan through its descriptor), for both slots of a pair.
template <bool PAIRS, bool SET, bool BYTES>
__device__ __forceinline__ void locate_tails(SLIME_RLOCATE_PARAMS, uint32_t* strip) {
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
    const Slots ps = column_slots<PAIRS, SET, BYTES>(in + (d->src_off << 2), cmp + (d->dst_off << 2), pl.coeff, iidx,
                                                     d->src_shard << 2, pl.oidx, d->dst_shard << 2, pl.rows, k, m,
                                                     it.col, rows, strip);
    if (ps.a != kNoSlot) {
      atomicAdd(counts + (uint64_t)it.obj * nslots + ps.a, 1ull);
      atomicMin(first + (uint64_t)it.obj * nslots + ps.a, (unsigned long long)it.col);
    }
    if constexpr (PAIRS) {
      if (ps.b != kNoSlot) {  // a pair: the column counts for both of its slots
        atomicAdd(counts + (uint64_t)it.obj * nslots + ps.b, 1ull);
        atomicMin(first + (uint64_t)it.obj * nslots + ps.b, (unsigned long long)it.col);
      }
    }
  }
}

// Four columns a lane, k = K <= 16 over 4-byte aligned bases: a static walk over the unit list,
// a tile in verify's steps of W vectors a lane, one step at a time.  With SET, R comes from the
// set's max_rows; row_bases and flag_tile clip to the object's own rows.  PAIRS: R is 4 (pair
// launches have rows >= 4).
template <bool PAIRS, int K, int W, int R, int UB, int C, bool SET, bool BYTES>
__device__ __forceinline__ void locate_vectors(SLIME_RLOCATE_PARAMS, uint32_t* strip) {
  static_assert(K > 0 && K <= 16 && W >= 1 && W <= UB && W <= 4, "compile-time k; a step is at most a tile");
  static_assert(!PAIRS || R == 4, "the pair kernels carry four stored rows a step");
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
        // Two branches with the same three source-side statements: in the one-shard SET kernels the
        // index line is read before them, in the pair SET kernels after them, as without SET.  The
        // statement order is what the kernels' machine code is compared by (tools/kernel_ids.py):
        // a shared tail behind the read changes both one-shard families' kernels, and the
        // one-shard order changes the pair SET kernels.
        if constexpr (SET && !PAIRS) {
          const PlanRef p = ragged::load_plan(coeff, descs, w.obj);
          pl = ragged::whole_plan(coeff, p);
          iidx = coeff + p.in_off;
          const u32x16 idx = *reinterpret_cast<const u32x16*>(iidx);  // K <= 16: one line
          if constexpr (BYTES) m = mapping[w.obj];  // wave-uniform
          ib = in + (w.d.src_off << 2);
          ishard = w.d.src_shard << 2;
#pragma unroll
          for (int j = 0; j < K; ++j) sb[j] = ib + (uint64_t)idx[j] * ishard;
        } else {
          if constexpr (BYTES) m = mapping[w.obj];  // wave-uniform
          ib = in + (w.d.src_off << 2);
          ishard = w.d.src_shard << 2;
          if constexpr (SET) {
            const PlanRef p = ragged::load_plan(coeff, descs, w.obj);
            pl = ragged::whole_plan(coeff, p);
            iidx = coeff + p.in_off;
            const u32x16 idx = *reinterpret_cast<const u32x16*>(iidx);  // K <= 16: one line
#pragma unroll
            for (int j = 0; j < K; ++j) sb[j] = ib + (uint64_t)idx[j] * ishard;
          } else {
#pragma unroll
            for (int j = 0; j < K; ++j) sb[j] = ib + (uint64_t)in_idx[j] * ishard;
          }
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
            // The one-shard kernels keep their scalar slot: through column_slots' Slots, as in
            // locate_tails and locate_columns, eight of them (BYTES, K <= 7) get other machine code.
            if constexpr (PAIRS) {
              Slots ps{kNoSlot, kNoSlot};
              if (hit)
                ps = column_slots<true, SET, BYTES>(ib, cb, pl.coeff, iidx, ishard, pl.oidx, cshard, pl.rows, k, m, col,
                                                    rows, strip);
              tally_slots(t, ps.a, col);
              tally_slots(t, ps.b, col);
            } else {
              uint32_t slot = kNoSlot;
              if (hit) {
                slot = classify_column<BYTES>(ib, cb, pl.coeff, iidx, ishard, pl.oidx, cshard, pl.rows, k, m, col);
                if constexpr (SET) slot = set_slot(slot, k, pl.rows, rows);
              }
              tally_slots(t, slot, col);
            }
          }
        }
      }
    }
    w.advance();
  }
  t.flush();
  locate_tails<PAIRS, SET, BYTES>(SLIME_RLOCATE_PASS, strip);
}

// One column a lane over the same unit list (static walk): generic k through wide_dot, any
// alignment; with SET the unit's object's plan is read per unit.  tile_cols = 256 UB,
// unit_tiles = C of the batch's geometry.
template <bool PAIRS, bool SET, bool BYTES>
__device__ __forceinline__ void locate_columns(SLIME_RLOCATE_PARAMS, uint32_t tile_cols, uint32_t unit_tiles,
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
    const ragged::ColRange c = ragged::unit_columns(d.ntiles, u, tile_cols, unit_tiles, d.nvec);
    unsigned long long* const res = counts + (uint64_t)u.obj * nslots;
    if (res != t.mism) {
      t.flush();
      t.begin(res, first + (uint64_t)u.obj * nslots);
    }
    const uint8_t* const ib = in + (d.src_off << 2);
    const uint8_t* const cb = cmp + (d.dst_off << 2);
    const uint64_t ishard = d.src_shard << 2, cshard = d.dst_shard << 2;
    for (uint64_t bw = c.b0; bw < c.b1; bw += 64) {
      // bw is always inside the object; lanes past the last column re-read column bw and never count.
      const bool ok = bw + lane < c.b1;
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
        if (bad)
          ps = column_slots<PAIRS, SET, BYTES>(ib, cb, pl.coeff, iidx, ishard, pl.oidx, cshard, pl.rows, k, m, col,
                                               rows, strip);
        tally_slots(t, ps.a, col);
        if constexpr (PAIRS) tally_slots(t, ps.b, col);
      }
    }
  }
  t.flush();
  locate_tails<PAIRS, SET, BYTES>(SLIME_RLOCATE_PASS, strip);
}

}  // namespace locate
}  // namespace slime
