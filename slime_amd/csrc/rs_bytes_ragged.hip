// Ragged byte objects for CDNA4 (gfx950): the ragged and planned launches of
// rs_ragged.hip and rs_verify_ragged.hip over STORED CHUNK BYTES instead of
// symbols (slime_rs_decode_objects_batch, slime_rs_planset_decode_objects_batch,
// slime_rs_verify_objects_batch, slime_rs_planset_verify_objects_batch).  A
// stored word is big-endian and XOR-ed with its object's mapping value
// (MapFromGF; rs_bytes_kernel.hpp): symbol = BE(word) ^ m going in, word =
// BE(symbol ^ m) going out, m = mapping[object] -- a different value for every
// object of the batch.
//
// Layout: the batch's tables (ragged_plan.hpp) are used as they are.  A
// descriptor's offsets and strides count 4-byte words of chunk bytes, so chunk
// c of an object starts at base + 4 (off + c shard) bytes and holds 4 L bytes:
// the same batch serves the symbol launches and these.
//
// Forms (SET: the plan-set twin of each kernel, one template):
//   k <= 16, 4-byte aligned bases: rs_decode_ragged_kernel<K, U, C, ...> and
//     rs_verify_bytes_ragged_kernel<K, W, R, ...>, four columns a lane over
//     UnitWalk (rs_ragged_walk.hpp) with the U, C, W and R of the symbol
//     kernels and their three walks: dynamic (tickets), static double-buffered
//     and static one tile at a time, chosen exactly as launch_apply_ragged and
//     launch_verify_ragged choose.
//   k > 16, or a base that is not 4-byte aligned: the column kernels, one
//     column a lane through apply::wide_dot over the same unit list (static
//     walk).  Correct for any k, not fast.
//
// The transform is applied where a tile's registers are CONSUMED (the first
// thing the store or compare step does), never where its loads are issued: the
// raw vectors of the next tile stay in flight through this tile's math, as in
// decode_bytes_pipe_kernel.  The transform reads every loaded register before
// any row math, so the waitcnt pass resolves a tile's loads there.
//
// The mapping belongs to the TILE, not to the walk.  The pipeline keeps two
// tiles live, the one being stored (compared) and the one being loaded, and
// after advance() they may belong to different objects with different
// mappings -- in the set forms with different plans too.  ByteTile and
// ByteStep therefore carry their own tile's mapping, plan rows and output
// base, fixed when the tile's loads are issued; the store or compare of the
// earlier tile never reads the walk's current object (`cur`, `cur_m`).
//
// Tails: the {object, column} items past the objects' last whole vectors are
// strided over the grid after the walk, one per lane, each with its own
// object's mapping (and plan).
//
// Verify rows: a launch tallies at most 64 rows; the host launches row blocks
// of 64 as rs_verify_ragged.hip does.  Only plain C++ vector stores and
// vector atomics write memory.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.hpp"
#include "planset_table.hpp"
#include "rs_apply_kernel.hpp"
#include "rs_bytes_kernel.hpp"  // load_raw_tile, rows_tile, be
#include "rs_ragged_walk.hpp"
#include "rs_verify_kernel.hpp"
#include "verify_step.hpp"

namespace slime {
namespace bytes_ragged {

using apply::kBlock;
using apply::kCoeffStride;
using apply::kWaves;
using apply::u32x16;
using bytes::be;
using ragged::Desc;
using ragged::ObjRef;
using ragged::PlanRef;
using ragged::Tail;
using ragged::Unit;
using ragged::UnitWalk;
using verify::Tally;

// A plan's rows as a launch reads them (verify: one row block of it).
struct PlanRows {
  const uint32_t* coeff;
  const uint32_t* oidx;
  uint32_t rows;
};

// raw chunk words -> symbols, in place: the first thing a tile's consumer does.
template <int K, int U>
__device__ __forceinline__ void to_symbols(uint4 (&x)[U][K], uint32_t m) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int j = 0; j < K; ++j)
      x[u][j] = make_uint4(be(x[u][j].x) ^ m, be(x[u][j].y) ^ m, be(x[u][j].z) ^ m, be(x[u][j].w) ^ m);
}

// ---- decode -------------------------------------------------------------------

// coeff: the plan's rows, or (SET) the set's table; in_idx / out_idx / rows: the plan's (unused by SET).
#define SLIME_BDECODE_PARAMS                                                                                         \
  const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const Desc *__restrict__ descs,                         \
      const Unit *__restrict__ units, const Tail *__restrict__ tails, const uint32_t *__restrict__ coeff,            \
      const uint32_t *__restrict__ in_idx, const uint32_t *__restrict__ out_idx,                                     \
      const uint32_t *__restrict__ mapping, uint32_t nunits, uint64_t ntails, uint32_t rows, uint32_t k

// Where a loaded tile goes and how it is read: its object's output base and
// chunk stride (bytes), vector count, the lane's first vector, and the
// object's mapping and plan.
struct ByteTile {
  uint8_t* ob;
  uint64_t shard;
  uint32_t nvec, g0;
  uint32_t m;
  PlanRows pl;
};

// One stored column (byte offset `off` into every chunk) of one object.
// K > 0: compile-time k, the inputs held in registers; K == 0: generic k.
template <int K>
__device__ __forceinline__ void decode_column(const uint8_t* ib, uint8_t* ob, const uint32_t* __restrict__ coeff,
                                              const uint32_t* __restrict__ in_idx, uint64_t in_shard,
                                              const uint32_t* __restrict__ out_idx, uint64_t out_shard, uint32_t rows,
                                              uint32_t k, uint32_t m, uint64_t off) {
  auto in_word = [&](uint32_t j) {
    return be(*reinterpret_cast<const uint32_t*>(ib + (uint64_t)in_idx[j] * in_shard + off)) ^ m;
  };
  uint32_t x[K > 0 ? K : 1];
  if constexpr (K > 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) x[j] = in_word(j);
  }
  for (uint32_t i = 0; i < rows; ++i) {
    uint32_t r;
    if constexpr (K > 0) {
      const apply::CoeffRow<K> c = apply::load_coeff_row<K>(coeff, i);
      uint64_t lo = 0;
      uint32_t hi = 0;
#pragma unroll
      for (int j = 0; j < K; ++j) mac(lo, hi, x[j], c[j]);
      r = fold96(lo, hi);
    } else {
      r = apply::wide_dot(coeff + (uint64_t)i * apply::wide_coeff_stride(k), k, in_word);
    }
    *reinterpret_cast<uint32_t*>(ob + (uint64_t)out_idx[i] * out_shard + off) = be(r ^ m);
  }
}

// The plan of object `obj` of a planned batch, whole (decode) -- pointers into the set's table.
__device__ __forceinline__ PlanRows set_plan(const uint32_t* __restrict__ tab, const Desc* d, const uint32_t** ii) {
  const uint32_t* const rec = tab + (uint64_t)d->reserved[0] * planset::kRecordWords;
  *ii = tab + rec[1];
  return PlanRows{tab + rec[3], tab + rec[2], rec[0]};
}

// The {object, column} items past the objects' last whole vectors, one per lane.
template <int K, bool SET>
__device__ __forceinline__ void decode_tails(SLIME_BDECODE_PARAMS) {
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t nthr = (uint64_t)gridDim.x * kBlock;
  for (uint64_t t = tid; t < ntails; t += nthr) {
    const Tail it = tails[t];
    const Desc* const d = descs + it.obj;
    PlanRows pl{coeff, out_idx, rows};
    const uint32_t* ii = in_idx;
    if constexpr (SET) pl = set_plan(coeff, d, &ii);
    decode_column<K>(in + (d->src_off << 2), out + (d->dst_off << 2), pl.coeff, ii, d->src_shard << 2, pl.oidx,
                     d->dst_shard << 2, pl.rows, k, mapping[it.obj], (uint64_t)it.col << 2);
  }
}

template <int K, int U, int C, int NC, bool DYN, bool PIPE, bool SET>
__global__ __launch_bounds__(kBlock) void rs_decode_ragged_kernel(SLIME_BDECODE_PARAMS,
                                                                  uint32_t* __restrict__ ticket) {
  static_assert(K > 0 && K <= 16 && NC > 0 && NC <= 64, "compile-time k only");
  static_assert(PIPE || !DYN, "the dynamic walk is double-buffered");
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  UnitWalk<C, NC, DYN> w(ticket, units, descs, nunits, lane, wave, gridDim.x * kWaves);
  // The walk's current object: read when a tile's loads are issued, never by a store.
  const uint8_t* sb[K];
  PlanRows cur{coeff, out_idx, rows};
  uint32_t cur_m = 0;
  auto bases = [&]() {
    u32x16 idx;
    if constexpr (SET) {
      const PlanRef pl = ragged::load_plan(coeff, descs, w.obj);
      cur = PlanRows{coeff + pl.coeff_off, coeff + pl.out_off, pl.rows};
      idx = *reinterpret_cast<const u32x16*>(coeff + pl.in_off);  // K <= 16: one line
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) idx[j] = in_idx[j];
    }
    cur_m = mapping[w.obj];  // wave-uniform: one scalar load
#pragma unroll
    for (int j = 0; j < K; ++j) sb[j] = in + ((w.d.src_off + (uint64_t)idx[j] * w.d.src_shard) << 2);
  };
  auto here = [&]() {
    return ByteTile{out + (w.d.dst_off << 2), w.d.dst_shard << 2, w.d.nvec, w.tile() * (64 * U) + lane, cur_m, cur};
  };
  auto load = [&](uint4(&x)[U][K], const ByteTile& t) { bytes::load_raw_tile<K, U>(x, sb, t.g0, t.nvec); };
  // The tile's OWN mapping and plan (t), whatever the walk has moved on to.
  auto store = [&](uint4(&x)[U][K], const ByteTile& t) {
    to_symbols<K, U>(x, t.m);
    bytes::rows_tile<K, U>(x, t.pl.rows, t.pl.coeff, t.pl.oidx, t.ob, t.shard, t.g0, t.nvec, t.m);
  };
  if constexpr (PIPE) {
    if (w.live) {
      uint4 xa[U][K], xb[U][K];
      bases();
      ByteTile ta = here(), tb = ta;
      load(xa, ta);
      for (;;) {
        w.advance();
        // Past the last unit the prefetch re-reads the current tile (unconditional loads, see load_raw_tile).
        tb = ta;
        if (w.live) {
          if (w.fresh) bases();
          tb = here();
        }
        load(xb, tb);
        store(xa, ta);  // ta's own mapping: bases() may just have moved cur_m on to tb's
        if (!w.live) break;
        w.advance();
        ta = tb;
        if (w.live) {
          if (w.fresh) bases();
          ta = here();
        }
        load(xa, ta);
        store(xb, tb);
        if (!w.live) break;
      }
    }
  } else {
    while (w.live) {
      uint4 x[U][K];
      if (w.fresh) bases();
      const ByteTile t = here();
      load(x, t);
      store(x, t);
      w.advance();
    }
  }
  w.finish();
  decode_tails<K, SET>(in, out, descs, units, tails, coeff, in_idx, out_idx, mapping, nunits, ntails, rows, k);
}

// One column per lane over the same unit list (static walk): generic k
// through wide_dot, any alignment.  tile_cols = 256 U, unit_tiles = C of the
// batch's geometry.
template <bool SET>
__global__ __launch_bounds__(kBlock) void rs_decode_ragged_column_kernel(SLIME_BDECODE_PARAMS, uint32_t tile_cols,
                                                                         uint32_t unit_tiles) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * kWaves;
  for (uint64_t e = wave; e < nunits; e += nwaves) {
    const Unit u = units[e];
    const ObjRef d = ragged::load_desc(descs, u.obj);
    PlanRows pl{coeff, out_idx, rows};
    const uint32_t* ii = in_idx;
    if constexpr (SET) {
      const PlanRef p = ragged::load_plan(coeff, descs, u.obj);
      pl = PlanRows{coeff + p.coeff_off, coeff + p.out_off, p.rows};
      ii = coeff + p.in_off;
    }
    const uint32_t m = mapping[u.obj];
    const uint32_t t1 = d.ntiles - u.tile < unit_tiles ? d.ntiles : u.tile + unit_tiles;
    const uint64_t b0 = (uint64_t)u.tile * tile_cols, bmax = (uint64_t)d.nvec << 2;
    const uint64_t b1 = (uint64_t)t1 * tile_cols < bmax ? (uint64_t)t1 * tile_cols : bmax;
    for (uint64_t b = b0 + lane; b < b1; b += 64)
      decode_column<0>(in + (d.src_off << 2), out + (d.dst_off << 2), pl.coeff, ii, d.src_shard << 2, pl.oidx,
                       d.dst_shard << 2, pl.rows, k, m, b << 2);
  }
  decode_tails<0, SET>(in, out, descs, units, tails, coeff, in_idx, out_idx, mapping, nunits, ntails, rows, k);
}

#undef SLIME_BDECODE_PARAMS

// ---- verify -------------------------------------------------------------------

// The rows of a plan that fall into the launch's row block [r0, r0 + 64).
__device__ __forceinline__ uint32_t block_rows(uint32_t rows, uint32_t r0) {
  return rows > r0 ? (rows - r0 < 64u ? rows - r0 : 64u) : 0u;
}

// Everything the compare of a step needs, fixed when the step's loads are issued.
struct ByteStep {
  const uint8_t* cb;  // the object's stored-chunk base (bytes) and chunk stride
  uint64_t cshard;
  unsigned long long* mism;  // the object's result rows
  unsigned long long* fst;
  PlanRows pl;      // the object's plan
  uint32_t m;       // the object's mapping
  uint32_t tb, v1;  // vectors [tb, tb + 64 W) of the object, clipped to v1
};

#define SLIME_BVERIFY_PARAMS                                                                                         \
  const uint8_t *__restrict__ in, const uint8_t *__restrict__ cmp, const Desc *__restrict__ descs,                   \
      const Unit *__restrict__ units, const Tail *__restrict__ tails, const uint32_t *__restrict__ coeff,            \
      const uint32_t *__restrict__ in_idx, const uint32_t *__restrict__ out_idx,                                     \
      const uint32_t *__restrict__ mapping, unsigned long long *__restrict__ mism,                                   \
      unsigned long long *__restrict__ first, uint32_t nunits, uint64_t ntails, uint32_t rows, uint32_t k,           \
      uint32_t r0, uint32_t res_stride

// The tail items: one {object, column} per lane, every row of the block, with
// the lane's own atomics (verify_tails, rs_verify_ragged.hip).
template <int K, bool SET>
__device__ __forceinline__ void verify_tails(SLIME_BVERIFY_PARAMS) {
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
    const uint32_t m = mapping[it.obj];
    const uint8_t* const ib = in + ((d->src_off + it.col) << 2);
    const uint8_t* const cb = cmp + ((d->dst_off + it.col) << 2);
    const uint64_t in_shard = d->src_shard << 2, cmp_shard = d->dst_shard << 2;
    auto in_word = [&](uint32_t j) {
      return be(*reinterpret_cast<const uint32_t*>(ib + (uint64_t)ii[j] * in_shard)) ^ m;
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
        const apply::CoeffRow<K> cr = apply::load_coeff_row<K>(c, i);
        uint64_t lo = 0;
        uint32_t hi = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) mac(lo, hi, x[j], cr[j]);
        r = fold96(lo, hi);
      } else {
        r = apply::wide_dot(c + (uint64_t)i * apply::wide_coeff_stride(k), k, in_word);
      }
      const uint32_t stored = *reinterpret_cast<const uint32_t*>(cb + (uint64_t)oi[i] * cmp_shard);
      if (stored != be(r ^ m)) {
        atomicAdd(mi + i, 1ull);
        atomicMin(f + i, (unsigned long long)it.col);
      }
    }
  }
}

// UB, C: the batch's geometry for K (vectors a lane a tile, tiles a unit);
// W: vectors a lane a step; R: stored rows loaded with a step's inputs
// (rs_verify_ragged_kernel's scheme, verify_step.hpp).
template <int K, int W, int R, int UB, int C, int NC, bool DYN, bool PIPE, bool SET>
__global__ __launch_bounds__(kBlock) void rs_verify_bytes_ragged_kernel(SLIME_BVERIFY_PARAMS,
                                                                        uint32_t* __restrict__ ticket) {
  static_assert(K > 0 && K <= 16 && NC > 0 && NC <= 64, "compile-time k only");
  static_assert(W >= 1 && W <= UB, "a step is at most a tile");
  static_assert(PIPE || !DYN, "the dynamic walk is double-buffered");
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  UnitWalk<C, NC, DYN> w(ticket, units, descs, nunits, lane, wave, gridDim.x * kWaves);
  Tally t(lane);
  // The walk's current object, plan and mapping: read when a step's loads are issued, never by a compare.
  const uint8_t* sb[K];
  const uint8_t* rb[R];
  const uint8_t* cb = nullptr;
  uint64_t cshard = 0, res = 0;
  PlanRows cur{coeff, out_idx, rows};
  uint32_t cur_m = 0;
  uint32_t st = 0, ns = 0, t0 = 0, tend = 0;  // the step inside the current tile, the tile's steps and vectors
  auto bases = [&]() {
    u32x16 idx;
    if constexpr (SET) {
      const PlanRef pl = ragged::load_plan(coeff, descs, w.obj);
      cur.rows = block_rows(pl.rows, r0);
      // No row in this block: the unit is passed over, and sb / rb keep the bases of the last
      // object that had loads (the prefetch past a wave's last step re-reads through them).
      if (cur.rows == 0) return;
      cur.coeff = coeff + pl.coeff_off + r0 * kCoeffStride;
      cur.oidx = coeff + pl.out_off + r0;
      idx = *reinterpret_cast<const u32x16*>(coeff + pl.in_off);  // K <= 16: one line
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) idx[j] = in_idx[j];
    }
    cur_m = mapping[w.obj];  // wave-uniform: one scalar load
#pragma unroll
    for (int j = 0; j < K; ++j) sb[j] = in + ((w.d.src_off + (uint64_t)idx[j] * w.d.src_shard) << 2);
    cb = cmp + (w.d.dst_off << 2);
    cshard = w.d.dst_shard << 2;
    res = (uint64_t)w.obj * res_stride;
    verify::row_bases<R>(rb, cb, cur.oidx, cshard, 0, cur.rows);
  };
  // After the walk moved: the new object's bases, units without a row in this block passed over,
  // and the steps of the tile the walk stands on.
  auto settle = [&]() {
    while (w.live) {
      if (w.fresh) bases();
      if (!SET || cur.rows != 0) break;
      w.advance();
    }
    if (w.live) {
      t0 = w.tile() * (64 * UB);
      tend = w.d.nvec - t0 < 64u * UB ? w.d.nvec : t0 + 64 * UB;  // the host lists tiles below nvec only
      ns = (tend - t0 + 64 * W - 1) / (64 * W);
      st = 0;
    }
  };
  auto next = [&]() {
    if (++st < ns) return;
    w.advance();
    settle();
  };
  auto here = [&]() { return ByteStep{cb, cshard, mism + res, first + res, cur, cur_m, t0 + st * (64 * W), tend}; };
  auto load = [&](uint4(&x)[W][K], uint4(&s)[R][W], const ByteStep& r) {
    verify::load_tile<K, W, R, uint32_t>(x, s, sb, rb, r.tb + lane, r.v1);
  };
  // The step's OWN object, plan and mapping (r), whatever the walk has moved on to.  check_tile
  // turns the raw inputs into symbols first and compares BE(computed ^ m) with the stored words.
  auto check = [&](uint4(&x)[W][K], uint4(&s)[R][W], const ByteStep& r) {
    if (r.mism != t.mism) {
      t.flush();
      t.begin(r.mism, r.fst);
    }
    verify::check_tile<K, W, R, true, uint32_t>(t, x, s, r.cb, r.pl.coeff, r.pl.oidx, r.cshard, r.pl.rows, r.m, r.tb,
                                                r.v1);
  };
  settle();
  if constexpr (PIPE) {
    if (w.live) {
      uint4 xa[W][K], xb[W][K], sa[R][W], sc[R][W];
      ByteStep ra = here(), rc = ra;
      load(xa, sa, ra);
      for (;;) {
        next();
        // Past the last step the prefetch re-reads the current one (unconditional loads, see load_tile).
        rc = ra;
        if (w.live) rc = here();
        load(xb, sc, rc);
        check(xa, sa, ra);
        if (!w.live) break;
        next();
        ra = rc;
        if (w.live) ra = here();
        load(xa, sa, ra);
        check(xb, sc, rc);
        if (!w.live) break;
      }
    }
  } else {
    while (w.live) {
      uint4 x[W][K], s[R][W];
      const ByteStep r = here();
      load(x, s, r);
      check(x, s, r);
      next();
    }
  }
  t.flush();
  w.finish();
  verify_tails<K, SET>(in, cmp, descs, units, tails, coeff, in_idx, out_idx, mapping, mism, first, nunits, ntails, rows,
                       k, r0, res_stride);
}

// One column per lane over the same unit list (static walk): generic k
// through wide_dot, any alignment.
template <bool SET>
__global__ __launch_bounds__(kBlock) void rs_verify_bytes_ragged_column_kernel(SLIME_BVERIFY_PARAMS,
                                                                               uint32_t tile_cols,
                                                                               uint32_t unit_tiles) {
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
    const uint32_t m = mapping[u.obj];
    const uint32_t t1 = d.ntiles - u.tile < unit_tiles ? d.ntiles : u.tile + unit_tiles;
    const uint64_t b0 = (uint64_t)u.tile * tile_cols, bmax = (uint64_t)d.nvec << 2;
    const uint64_t b1 = (uint64_t)t1 * tile_cols < bmax ? (uint64_t)t1 * tile_cols : bmax;
    unsigned long long* const mi = mism + (uint64_t)u.obj * res_stride;
    if (mi != t.mism) {
      t.flush();
      t.begin(mi, first + (uint64_t)u.obj * res_stride);
    }
    for (uint64_t bw = b0; bw < b1; bw += 64)
      verify::check_columns<0, true>(t, in + (d.src_off << 2), cmp + (d.dst_off << 2), pl.coeff, ii, d.src_shard << 2,
                                     pl.oidx, d.dst_shard << 2, pl.rows, k, m, bw, b1);
  }
  t.flush();
  verify_tails<0, SET>(in, cmp, descs, units, tails, coeff, in_idx, out_idx, mapping, mism, first, nunits, ntails, rows,
                       k, r0, res_stride);
}

#undef SLIME_BVERIFY_PARAMS

}  // namespace bytes_ragged

namespace {

using apply::kBlock;
constexpr uint64_t kQueueBlocks = 256;  // one block per CU, as the ragged apply launch

// Blocks of a launch: one wave per unit up to `full`, and enough lanes for
// the tail items of a batch of many short objects (rs_ragged.hip, ragged_blocks).
uint64_t ragged_blocks(uint64_t full, uint64_t nunits, uint64_t ntails) {
  const uint64_t by_units = queue_blocks(full, nunits);
  const uint64_t by_tails = (ntails + kBlock - 1) / kBlock;
  const uint64_t want = by_tails < full ? by_tails : full;
  return by_units > want ? by_units : want;
}

// f(std::integral_constant<int, K>) for the launch's k in 1 ... 16.
template <class F>
hipError_t with_k(uint32_t k, F&& f) {
  switch (k) {
#define SLIME_K(n) \
  case n: return f(std::integral_constant<int, n>{});
    SLIME_K(1) SLIME_K(2) SLIME_K(3) SLIME_K(4) SLIME_K(5) SLIME_K(6) SLIME_K(7) SLIME_K(8)
    SLIME_K(9) SLIME_K(10) SLIME_K(11) SLIME_K(12) SLIME_K(13) SLIME_K(14) SLIME_K(15)
#undef SLIME_K
    default: return f(std::integral_constant<int, 16>{});
  }
}

// ---- decode launches: the grids and the choice between the schedules are
// launch_apply_ragged's (rs_ragged.hip) ----

#define SLIME_BDECODE_ARGS(a, SET)                                                                        \
  (a).in, (a).out, (a).desc, (a).units, (a).tails, (SET) ? (a).table : (a).coeff, (a).in_idx, (a).out_idx, \
      (a).mapping, (a).nunits, (a).ntails, (a).rows, (a).k

template <int K, bool SET, bool PIPE>
hipError_t decode_static(const RaggedBytesLaunch& a, hipStream_t s) {
  constexpr int U = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K);
  const uint64_t blocks = ragged_blocks(K <= 12 ? 256 : 1024, a.nunits, a.ntails);
  hipLaunchKernelGGL((bytes_ragged::rs_decode_ragged_kernel<K, U, C, kQueueCounters, false, PIPE, SET>),
                     dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_BDECODE_ARGS(a, SET), nullptr);
  return hipGetLastError();
}

template <int K, bool SET>
hipError_t decode_dispatch(const RaggedBytesLaunch& a, hipStream_t s) {
  constexpr int U = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K);
  if (!pipelined_kernels()) return decode_static<K, SET, false>(a, s);
  // The dynamic schedule has nothing to balance over one block's units (queue_spread, kernels.hpp).
  if (queue_allowed(s) && a.nunits > tiny_queue_units()) {
    bool launched = false;
    const uint64_t blocks = ragged_blocks(kQueueBlocks, a.nunits, a.ntails);
    const hipError_t e = with_tickets(
        s,
        [&](uint32_t* set) {
          hipLaunchKernelGGL((bytes_ragged::rs_decode_ragged_kernel<K, U, C, kQueueCounters, true, true, SET>),
                             dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_BDECODE_ARGS(a, SET), set);
          return hipGetLastError();
        },
        &launched);
    if (launched || e != hipSuccess) return e;
  }
  return decode_static<K, SET, true>(a, s);
}

template <bool SET>
hipError_t decode_columns(const RaggedBytesLaunch& a, hipStream_t s) {
  const uint64_t blocks = ragged_blocks(1024, a.nunits, a.ntails);
  hipLaunchKernelGGL(bytes_ragged::rs_decode_ragged_column_kernel<SET>, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                     SLIME_BDECODE_ARGS(a, SET), 256u * (uint32_t)a.U, (uint32_t)a.C);
  return hipGetLastError();
}

#undef SLIME_BDECODE_ARGS

// ---- verify launches: launch_verify_ragged's (rs_verify_ragged.hip) ----

// One row block [r0, r0 + rows_c) of the launch.  Single plan: the plan's
// pointers moved on to the block; set: the table and r0.
struct Block {
  const RaggedBytesVerifyLaunch& v;
  uint32_t r0, rows_c;
};

#define SLIME_BVERIFY_ARGS(b, SET)                                                                                   \
  (b).v.in, (b).v.cmp, (b).v.desc, (b).v.units, (b).v.tails,                                                         \
      (SET) ? (b).v.table : (b).v.coeff + (uint64_t)(b).r0 * coeff_stride((b).v.k), (b).v.in_idx,                   \
      (SET) ? (const uint32_t*)nullptr : (b).v.out_idx + (b).r0, (b).v.mapping,                                      \
      (unsigned long long*)(b).v.mismatches + (b).r0, (unsigned long long*)(b).v.first + (b).r0, (b).v.nunits,       \
      (b).v.ntails, (SET) ? 0u : (b).rows_c, (b).v.k, (SET) ? (b).r0 : 0u, (b).v.rows

template <int K, int R, bool SET, bool PIPE>
hipError_t verify_static(const Block& b, hipStream_t s) {
  constexpr int UB = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K), W = verify_step::width(K, R);
  // Fat waves one block a CU, thin ones (one vector a lane) four, as the uniform verify launch.
  const uint64_t blocks = ragged_blocks(W == 1 ? 1024 : 256, b.v.nunits, b.v.ntails);
  hipLaunchKernelGGL((bytes_ragged::rs_verify_bytes_ragged_kernel<K, W, R, UB, C, kQueueCounters, false, PIPE, SET>),
                     dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_BVERIFY_ARGS(b, SET), nullptr);
  return hipGetLastError();
}

template <int K, int R, bool SET>
hipError_t verify_dispatch(const Block& b, hipStream_t s) {
  constexpr int UB = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K), W = verify_step::width(K, R);
  if (!pipelined_kernels()) return verify_static<K, R, SET, false>(b, s);
  if (queue_allowed(s) && b.v.nunits > tiny_queue_units()) {
    bool launched = false;
    const uint64_t blocks = ragged_blocks(kQueueBlocks, b.v.nunits, b.v.ntails);
    const hipError_t e = with_tickets(
        s,
        [&](uint32_t* set) {
          hipLaunchKernelGGL(
              (bytes_ragged::rs_verify_bytes_ragged_kernel<K, W, R, UB, C, kQueueCounters, true, true, SET>),
              dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_BVERIFY_ARGS(b, SET), set);
          return hipGetLastError();
        },
        &launched);
    if (launched || e != hipSuccess) return e;
  }
  return verify_static<K, R, SET, true>(b, s);
}

template <int K>
hipError_t verify_rows(const Block& b, hipStream_t s) {
  const bool set = b.v.table != nullptr;
  if (verify_step::stored_rows(b.rows_c) == 2)
    return set ? verify_dispatch<K, 2, true>(b, s) : verify_dispatch<K, 2, false>(b, s);
  return set ? verify_dispatch<K, 4, true>(b, s) : verify_dispatch<K, 4, false>(b, s);
}

hipError_t verify_columns(const Block& b, hipStream_t s) {
  const uint64_t blocks = ragged_blocks(1024, b.v.nunits, b.v.ntails);
  if (b.v.table)
    hipLaunchKernelGGL(bytes_ragged::rs_verify_bytes_ragged_column_kernel<true>, dim3((uint32_t)blocks), dim3(kBlock),
                       0, s, SLIME_BVERIFY_ARGS(b, true), 256u * (uint32_t)b.v.U, (uint32_t)b.v.C);
  else
    hipLaunchKernelGGL(bytes_ragged::rs_verify_bytes_ragged_column_kernel<false>, dim3((uint32_t)blocks),
                       dim3(kBlock), 0, s, SLIME_BVERIFY_ARGS(b, false), 256u * (uint32_t)b.v.U, (uint32_t)b.v.C);
  return hipGetLastError();
}

#undef SLIME_BVERIFY_ARGS

}  // namespace

hipError_t launch_decode_bytes_ragged(const RaggedBytesLaunch& a, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (a.nunits == 0 && a.ntails == 0) return hipSuccess;
  const bool set = a.table != nullptr;
  if (!set && a.rows == 0) return hipSuccess;
  if (a.k > 16 || !a.vec_ok) return set ? decode_columns<true>(a, s) : decode_columns<false>(a, s);
  // The vector kernels are instantiated with the geometry of their K: the tables must be cut by it.
  if (a.U != ragged::unroll_for_k((int)a.k) || a.C != ragged::unit_tiles_for_k((int)a.k)) return hipErrorInvalidValue;
  return with_k(a.k, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    return set ? decode_dispatch<K, true>(a, s) : decode_dispatch<K, false>(a, s);
  });
}

hipError_t launch_verify_bytes_ragged(const RaggedBytesVerifyLaunch& v, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (v.nobj == 0 || v.rows == 0) return hipSuccess;
  if (hipError_t e = launch_verify_init(v.mismatches, v.first, v.nobj * v.rows, s)) return e;
  if (v.nunits == 0 && v.ntails == 0) return hipSuccess;  // an empty batch: nothing but the initialisation
  const bool vec = v.k <= 16 && v.vec_ok;
  if (vec && (v.U != ragged::unroll_for_k((int)v.k) || v.C != ragged::unit_tiles_for_k((int)v.k)))
    return hipErrorInvalidValue;
  // A launch tallies at most 64 rows (one lane each): larger plans and sets go in row blocks.
  for (uint32_t r0 = 0; r0 < v.rows; r0 += 64) {
    const Block b{v, r0, v.rows - r0 < 64 ? v.rows - r0 : 64};
    const hipError_t e = vec ? with_k(v.k,
                                      [&](auto kc) {
                                        constexpr int K = decltype(kc)::value;
                                        return verify_rows<K>(b, s);
                                      })
                             : verify_columns(b, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace slime
