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
#include "rs_ragged_walk.hpp"
#include "rs_verify_kernel.hpp"
#include "verify_step.hpp"

namespace slime {
namespace verify {

using apply::kCoeffStride;
using apply::u32x16;
using ragged::Desc;
using ragged::ObjRef;
using ragged::PlanRef;
using ragged::Tail;
using ragged::Unit;
using ragged::UnitWalk;

// The rows of a plan that fall into the launch's row block [r0, r0 + 64).
__device__ __forceinline__ uint32_t block_rows(uint32_t rows, uint32_t r0) {
  return rows > r0 ? (rows - r0 < 64u ? rows - r0 : 64u) : 0u;
}

// A plan as one row block of a launch reads it.
struct PlanRows {
  const uint32_t* coeff;
  const uint32_t* oidx;
  uint32_t rows;
};

// Everything the compare of a step needs, fixed when the step's loads are issued.
struct StepRef {
  const uint8_t* cb;  // the object's stored-row base (bytes) and shard stride
  uint64_t cshard;
  unsigned long long* mism;  // the object's result rows
  unsigned long long* fst;
  PlanRows pl;       // the object's plan
  uint32_t tb, v1;   // vectors [tb, tb + 64 W) of the object, clipped to v1
};

#define SLIME_RVERIFY_PARAMS                                                                                         \
  const uint8_t *__restrict__ in, const uint8_t *__restrict__ cmp, const Desc *__restrict__ descs,                   \
      const Unit *__restrict__ units, const Tail *__restrict__ tails, const uint32_t *__restrict__ coeff,            \
      const uint32_t *__restrict__ in_idx, const uint32_t *__restrict__ out_idx,                                     \
      unsigned long long *__restrict__ mism, unsigned long long *__restrict__ first, uint32_t nunits,                \
      uint64_t ntails, uint32_t rows, uint32_t k, uint32_t r0, uint32_t res_stride

// The tail items: one {object, column} per lane, every row of the block.
// SET: `coeff` is the set's table and the item's plan comes through its
// descriptor.  K == 0: generic k.
template <int K, bool SET>
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
    const uint8_t* const ib = in + ((d->src_off + it.col) << 2);
    const uint8_t* const cb = cmp + ((d->dst_off + it.col) << 2);
    const uint64_t in_shard = d->src_shard << 2, cmp_shard = d->dst_shard << 2;
    auto in_word = [&](uint32_t j) { return *reinterpret_cast<const uint32_t*>(ib + (uint64_t)ii[j] * in_shard); };
    unsigned long long* const m = mism + (uint64_t)it.obj * res_stride;
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
      if (stored != r) {
        atomicAdd(m + i, 1ull);
        atomicMin(f + i, (unsigned long long)it.col);
      }
    }
  }
}

// UB, C: the batch's geometry for K (vectors a lane a tile, tiles a unit);
// W: vectors a lane a step; R: stored rows loaded with a step's inputs.
template <int K, int W, int R, int UB, int C, int NC, bool DYN, bool PIPE, bool SET>
__global__ __launch_bounds__(kBlock) void rs_verify_ragged_kernel(SLIME_RVERIFY_PARAMS, uint32_t* __restrict__ ticket) {
  static_assert(K > 0 && K <= 16 && NC > 0 && NC <= 64, "compile-time k only");
  static_assert(W >= 1 && W <= UB, "a step is at most a tile");
  static_assert(PIPE || !DYN, "the dynamic walk is double-buffered");
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  UnitWalk<C, NC, DYN> w(ticket, units, descs, nunits, lane, wave, gridDim.x * kWaves);
  Tally t(lane);
  // The walk's current object and plan: read when a step's loads are issued, never by a compare.
  const uint8_t* sb[K];
  const uint8_t* rb[R];
  const uint8_t* cb = nullptr;
  uint64_t cshard = 0, res = 0;
  PlanRows cur{coeff, out_idx, rows};
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
#pragma unroll
    for (int j = 0; j < K; ++j) sb[j] = in + ((w.d.src_off + (uint64_t)idx[j] * w.d.src_shard) << 2);
    cb = cmp + (w.d.dst_off << 2);
    cshard = w.d.dst_shard << 2;
    res = (uint64_t)w.obj * res_stride;
    row_bases<R>(rb, cb, cur.oidx, cshard, 0, cur.rows);
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
  auto here = [&]() { return StepRef{cb, cshard, mism + res, first + res, cur, t0 + st * (64 * W), tend}; };
  auto load = [&](uint4(&x)[W][K], uint4(&s)[R][W], const StepRef& r) {
    load_tile<K, W, R, uint32_t>(x, s, sb, rb, r.tb + lane, r.v1);
  };
  // The step's OWN object and plan (r), whatever the walk has moved on to.
  auto check = [&](uint4(&x)[W][K], uint4(&s)[R][W], const StepRef& r) {
    if (r.mism != t.mism) {
      t.flush();
      t.begin(r.mism, r.fst);
    }
    check_tile<K, W, R, false, uint32_t>(t, x, s, r.cb, r.pl.coeff, r.pl.oidx, r.cshard, r.pl.rows, 0u, r.tb, r.v1);
  };
  settle();
  if constexpr (PIPE) {
    if (w.live) {
      uint4 xa[W][K], xb[W][K], sa[R][W], sc[R][W];
      StepRef ra = here(), rc = ra;
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
      const StepRef r = here();
      load(x, s, r);
      check(x, s, r);
      next();
    }
  }
  t.flush();
  w.finish();
  verify_tails<K, SET>(in, cmp, descs, units, tails, coeff, in_idx, out_idx, mism, first, nunits, ntails, rows, k, r0,
                       res_stride);
}

// One column per lane over the same unit list (static walk): generic k
// through wide_dot, any alignment.  tile_cols = 256 UB, unit_tiles = C of the
// batch's geometry.
template <bool SET>
__global__ __launch_bounds__(kBlock) void rs_verify_ragged_column_kernel(SLIME_RVERIFY_PARAMS, uint32_t tile_cols,
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
    const uint32_t t1 = d.ntiles - u.tile < unit_tiles ? d.ntiles : u.tile + unit_tiles;
    const uint64_t b0 = (uint64_t)u.tile * tile_cols, bmax = (uint64_t)d.nvec << 2;
    const uint64_t b1 = (uint64_t)t1 * tile_cols < bmax ? (uint64_t)t1 * tile_cols : bmax;
    unsigned long long* const m = mism + (uint64_t)u.obj * res_stride;
    if (m != t.mism) {
      t.flush();
      t.begin(m, first + (uint64_t)u.obj * res_stride);
    }
    for (uint64_t bw = b0; bw < b1; bw += 64)
      check_columns<0, false>(t, in + (d.src_off << 2), cmp + (d.dst_off << 2), pl.coeff, ii, d.src_shard << 2, pl.oidx,
                              d.dst_shard << 2, pl.rows, k, 0u, bw, b1);
  }
  t.flush();
  verify_tails<0, SET>(in, cmp, descs, units, tails, coeff, in_idx, out_idx, mism, first, nunits, ntails, rows, k, r0,
                       res_stride);
}

#undef SLIME_RVERIFY_PARAMS

}  // namespace verify

namespace {

using apply::kBlock;
constexpr uint64_t kQueueBlocks = 256;  // one block per CU, as the ragged apply launch

// Blocks of a launch: one wave per unit up to `full`, and enough lanes for
// the tail items of a batch of many short objects (rs_ragged.hip, ragged_blocks).
uint64_t ragged_blocks(uint64_t full, const RaggedVerifyLaunch& v) {
  const uint64_t by_units = queue_blocks(full, v.nunits);
  const uint64_t by_tails = (v.ntails + kBlock - 1) / kBlock;
  const uint64_t want = by_tails < full ? by_tails : full;
  return by_units > want ? by_units : want;
}

// One row block [r0, r0 + rows_c) of the launch.  Single plan: the plan's
// pointers moved on to the block; set: the table and r0.
struct Block {
  const RaggedVerifyLaunch& v;
  uint32_t r0, rows_c;
};

#define SLIME_RVERIFY_ARGS(b, SET)                                                                                   \
  (const uint8_t*)(b).v.in, (const uint8_t*)(b).v.cmp, (b).v.desc, (b).v.units, (b).v.tails,                         \
      (SET) ? (b).v.table : (b).v.coeff + (uint64_t)(b).r0 * coeff_stride((b).v.k), (b).v.in_idx,                   \
      (SET) ? (const uint32_t*)nullptr : (b).v.out_idx + (b).r0, (unsigned long long*)(b).v.mismatches + (b).r0,     \
      (unsigned long long*)(b).v.first + (b).r0, (b).v.nunits, (b).v.ntails, (SET) ? 0u : (b).rows_c, (b).v.k,       \
      (SET) ? (b).r0 : 0u, (b).v.rows

template <int K, int R, bool SET, bool PIPE>
hipError_t launch_static(const Block& b, hipStream_t s) {
  constexpr int UB = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K), W = verify_step::width(K, R);
  // Fat waves one block a CU, thin ones (one vector a lane) four, as the uniform verify launch.
  const uint64_t blocks = ragged_blocks(W == 1 ? 1024 : 256, b.v);
  hipLaunchKernelGGL((verify::rs_verify_ragged_kernel<K, W, R, UB, C, kQueueCounters, false, PIPE, SET>),
                     dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_RVERIFY_ARGS(b, SET), nullptr);
  return hipGetLastError();
}

// The choice between the schedules is launch_apply_ragged's (rs_ragged.hip, dispatch).
template <int K, int R, bool SET>
hipError_t dispatch(const Block& b, hipStream_t s) {
  constexpr int UB = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K), W = verify_step::width(K, R);
  if (!pipelined_kernels()) return launch_static<K, R, SET, false>(b, s);
  if (queue_allowed(s) && b.v.nunits > tiny_queue_units()) {
    bool launched = false;
    const uint64_t blocks = ragged_blocks(kQueueBlocks, b.v);
    const hipError_t e = with_tickets(
        s,
        [&](uint32_t* set) {
          hipLaunchKernelGGL((verify::rs_verify_ragged_kernel<K, W, R, UB, C, kQueueCounters, true, true, SET>),
                             dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_RVERIFY_ARGS(b, SET), set);
          return hipGetLastError();
        },
        &launched);
    if (launched || e != hipSuccess) return e;
  }
  return launch_static<K, R, SET, true>(b, s);
}

template <int K>
hipError_t dispatch_rows(const Block& b, hipStream_t s) {
  const bool set = b.v.table != nullptr;
  if (verify_step::stored_rows(b.rows_c) == 2) return set ? dispatch<K, 2, true>(b, s) : dispatch<K, 2, false>(b, s);
  return set ? dispatch<K, 4, true>(b, s) : dispatch<K, 4, false>(b, s);
}

hipError_t launch_columns(const Block& b, hipStream_t s) {
  const uint64_t blocks = ragged_blocks(1024, b.v);
  if (b.v.table)
    hipLaunchKernelGGL(verify::rs_verify_ragged_column_kernel<true>, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                       SLIME_RVERIFY_ARGS(b, true), 256u * (uint32_t)b.v.U, (uint32_t)b.v.C);
  else
    hipLaunchKernelGGL(verify::rs_verify_ragged_column_kernel<false>, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                       SLIME_RVERIFY_ARGS(b, false), 256u * (uint32_t)b.v.U, (uint32_t)b.v.C);
  return hipGetLastError();
}

#undef SLIME_RVERIFY_ARGS

hipError_t launch_block(const Block& b, hipStream_t s) {
  if (b.v.k > 16 || !b.v.vec_ok) return launch_columns(b, s);
  switch (b.v.k) {
    case 1: return dispatch_rows<1>(b, s);
    case 2: return dispatch_rows<2>(b, s);
    case 3: return dispatch_rows<3>(b, s);
    case 4: return dispatch_rows<4>(b, s);
    case 5: return dispatch_rows<5>(b, s);
    case 6: return dispatch_rows<6>(b, s);
    case 7: return dispatch_rows<7>(b, s);
    case 8: return dispatch_rows<8>(b, s);
    case 9: return dispatch_rows<9>(b, s);
    case 10: return dispatch_rows<10>(b, s);
    case 11: return dispatch_rows<11>(b, s);
    case 12: return dispatch_rows<12>(b, s);
    case 13: return dispatch_rows<13>(b, s);
    case 14: return dispatch_rows<14>(b, s);
    case 15: return dispatch_rows<15>(b, s);
    default: return dispatch_rows<16>(b, s);
  }
}

}  // namespace

hipError_t launch_verify_ragged(const RaggedVerifyLaunch& v, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (v.nobj == 0 || v.rows == 0) return hipSuccess;
  if (hipError_t e = launch_verify_init(v.mismatches, v.first, v.nobj * v.rows, s)) return e;
  if (v.nunits == 0 && v.ntails == 0) return hipSuccess;  // an empty batch: nothing but the initialisation
  // The vector kernels are instantiated with the geometry of their K: the tables must be cut by it.
  if (v.k <= 16 && v.vec_ok &&
      (v.U != ragged::unroll_for_k((int)v.k) || v.C != ragged::unit_tiles_for_k((int)v.k)))
    return hipErrorInvalidValue;
  // A launch tallies at most 64 rows (one lane each): larger plans and sets go in row blocks.
  for (uint32_t r0 = 0; r0 < v.rows; r0 += 64) {
    const Block b{v, r0, v.rows - r0 < 64 ? v.rows - r0 : 64};
    if (hipError_t e = launch_block(b, s)) return e;
  }
  return hipSuccess;
}

}  // namespace slime
