// Ragged batches for CDNA4 (gfx950): one launch of a plan over objects of
// different lengths at arbitrary offsets (slime_rs_plan_execute_batch).  The
// arithmetic and the tile loads and stores are rs_apply_kernel.hpp's
// (load_tile, store_tile, apply_column); what is new is where a wave's work
// comes from.  The host (ragged_plan.hpp) cuts every object into units of up
// to C consecutive tiles of 256 U columns and lists them, {object, first
// tile}, in device memory beside one 64-byte descriptor per object; a unit
// never crosses an object, and the list goes round the objects four units at
// a time.
//
// Forms (a batch serves every plan with its k inputs on its device):
//   k <= 16, 4-byte aligned src and dst: rs_apply_ragged_kernel<K, U, C>, four
//     columns a lane, U and C as the dynamic-schedule apply launch picks them
//     for K.  DYN: units are tickets drawn from the eight per-XCD counters of
//     a counter set exactly as TicketWalk draws them (rs_apply_kernel.hpp:
//     empty partitions passed over, the exit counter, the last wave out zeroes
//     the set); ticket l of partition p is list entry ((l / 4) NC + p) 4 + l % 4,
//     so the four waves that take consecutive tickets sweep four consecutive
//     units of one object, and the next group belongs to the next object.  Static (schedule mode 0, captures under mode 1, no counter set
//     to be had, batches of at most SLIME_RS_TINY_UNITS units): wave w takes
//     entries w, w + nwaves, ...  Both double-buffered; slime_rs_kernel_pipeline(0)
//     runs the static walk one tile at a time.
//   k > 16, or a base that is not 4-byte aligned: rs_apply_ragged_column_kernel,
//     one column per lane through apply::wide_dot over the same unit list
//     (static walk).  Correct for any k a plan allows; matrix-core and
//     k-template ragged kernels are out of scope.
//
// The walk keeps two things in flight: the ticket for the unit after the
// next (an atomic, lane 0) and the list entry of the next unit (one 8-byte
// scalar load), each issued a unit before it is read.  On entering a unit of
// another object the wave takes that object's descriptor (one
// s_load_dwordx16) and recomputes its K input bases and its output base,
// wave-uniform SGPR pairs; inside the double-buffered loop nothing else
// differs from rs_apply_queue_kernel: loads are unconditional, lanes past the
// object's last vector re-read it, the prefetch past a wave's last unit
// re-reads its current tile.
//
// Columns past each object's last whole vector (L % 4; all of an object of
// fewer than 4 columns) are {object, column} items strided over the grid
// after the walk, one per lane, through apply_column<K>.
//
// Plan sets (slime_rs_planset_execute_batch): rs_apply_planned_kernel and
// rs_apply_planned_column_kernel below are the twins of the two kernels with a
// plan PER OBJECT, named by the object's descriptor and read from a plan set's
// table (planset_table.hpp).  The single-plan kernels are unchanged.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "planset_table.hpp"
#include "rs_apply_kernel.hpp"
#include "rs_ragged_launch.hpp"  // the grid, with_k and the choice between the schedules
#include "rs_ragged_walk.hpp"    // UnitWalk, load_desc, load_plan: shared with rs_verify_ragged.hip

namespace slime {
namespace ragged {

// Where a loaded tile goes: its object's output base and stride, the
// object's vector count and the lane's first vector.
struct TileOut {
  uint32_t* ob;
  uint64_t shard;
  uint32_t nvec, g0;
};

// The {object, column} items past the objects' last whole vectors, strided
// over the grid, one per lane (K == 0: generic k).
template <int K>
__device__ __forceinline__ void ragged_tails(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                             const Desc* __restrict__ descs, const Tail* __restrict__ tails,
                                             uint64_t ntails, const uint32_t* __restrict__ coeff,
                                             const uint32_t* __restrict__ in_idx,
                                             const uint32_t* __restrict__ out_idx, uint32_t rows, uint32_t k) {
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t nthr = (uint64_t)gridDim.x * kBlock;
  for (uint64_t t = tid; t < ntails; t += nthr) {
    const Tail it = tails[t];
    const Desc* const d = descs + it.obj;
    apply::apply_column<K>(in + d->src_off, out + d->dst_off, coeff, in_idx, d->src_shard, out_idx, d->dst_shard,
                           rows, k, (uint64_t)it.col);
  }
}

template <int K, int U, int C, int NC, bool NTL, bool NTS, bool DYN, bool PIPE>
__global__ __launch_bounds__(kBlock) void rs_apply_ragged_kernel(
    const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const Desc* __restrict__ descs,
    const Unit* __restrict__ units, const Tail* __restrict__ tails, const uint32_t* __restrict__ coeff,
    const uint32_t* __restrict__ in_idx, const uint32_t* __restrict__ out_idx, uint32_t nunits, uint64_t ntails,
    uint32_t rows, uint32_t k, uint32_t* __restrict__ ticket) {
  static_assert(K > 0 && K <= 16 && NC > 0 && NC <= 64, "compile-time k only");
  static_assert(PIPE || !DYN, "the dynamic walk is double-buffered");
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  UnitWalk<C, NC, DYN> w(ticket, units, descs, nunits, lane, wave, gridDim.x * kWaves);
  const uint32_t* sb[K];
  auto bases = [&]() {
#pragma unroll
    for (int j = 0; j < K; ++j) sb[j] = in + w.d.src_off + (uint64_t)in_idx[j] * w.d.src_shard;
  };
  auto here = [&]() { return TileOut{out + w.d.dst_off, w.d.dst_shard, w.d.nvec, w.tile() * (64 * U) + lane}; };
  if constexpr (PIPE) {
    if (w.live) {
      uint4 xa[U][K], xb[U][K];
      bases();
      TileOut ta = here(), tb = ta;
      apply::load_tile<K, U, NTL>(xa, sb, ta.g0, ta.nvec);
      for (;;) {
        w.advance();
        // Past the last unit the prefetch re-reads the current tile (unconditional loads, see load_tile).
        tb = ta;
        if (w.live) {
          if (w.fresh) bases();
          tb = here();
        }
        apply::load_tile<K, U, NTL>(xb, sb, tb.g0, tb.nvec);
        apply::store_tile<K, U, NTS>(xa, ta.ob, coeff, out_idx, ta.shard, rows, ta.g0, ta.nvec);
        if (!w.live) break;
        w.advance();
        ta = tb;
        if (w.live) {
          if (w.fresh) bases();
          ta = here();
        }
        apply::load_tile<K, U, NTL>(xa, sb, ta.g0, ta.nvec);
        apply::store_tile<K, U, NTS>(xb, tb.ob, coeff, out_idx, tb.shard, rows, tb.g0, tb.nvec);
        if (!w.live) break;
      }
    }
  } else {
    while (w.live) {
      uint4 x[U][K];
      if (w.fresh) bases();
      const TileOut t = here();
      apply::load_tile<K, U, NTL>(x, sb, t.g0, t.nvec);
      apply::store_tile<K, U, NTS>(x, t.ob, coeff, out_idx, t.shard, rows, t.g0, t.nvec);
      w.advance();
    }
  }
  w.finish();
  ragged_tails<K>(in, out, descs, tails, ntails, coeff, in_idx, out_idx, rows, k);
}

// One column per lane over the same unit list (static walk): generic k
// through wide_dot, any alignment.  tile_cols = 256 U, unit_tiles = C of the
// batch's geometry.
__global__ __launch_bounds__(kBlock) void rs_apply_ragged_column_kernel(
    const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const Desc* __restrict__ descs,
    const Unit* __restrict__ units, const Tail* __restrict__ tails, const uint32_t* __restrict__ coeff,
    const uint32_t* __restrict__ in_idx, const uint32_t* __restrict__ out_idx, uint32_t nunits, uint64_t ntails,
    uint32_t rows, uint32_t k, uint32_t tile_cols, uint32_t unit_tiles) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * kWaves;
  for (uint64_t e = wave; e < nunits; e += nwaves) {
    const Unit u = units[e];
    const ObjRef d = load_desc(descs, u.obj);
    const uint32_t t1 = d.ntiles - u.tile < unit_tiles ? d.ntiles : u.tile + unit_tiles;
    const uint64_t b0 = (uint64_t)u.tile * tile_cols, bmax = (uint64_t)d.nvec << 2;
    const uint64_t b1 = (uint64_t)t1 * tile_cols < bmax ? (uint64_t)t1 * tile_cols : bmax;
    for (uint64_t b = b0 + lane; b < b1; b += 64)
      apply::apply_column<0>(in + d.src_off, out + d.dst_off, coeff, in_idx, d.src_shard, out_idx, d.dst_shard, rows,
                             k, b);
  }
  ragged_tails<0>(in, out, descs, tails, ntails, coeff, in_idx, out_idx, rows, k);
}

// ---- plan sets: every object its own plan (slime_rs_planset_execute_batch) ----
// The planned twins of the two kernels above.  The batch's descriptors carry a
// plan index (Desc::reserved[0]); `tab` is the set's table (planset_table.hpp):
// the 64-byte record of plan i at word 16 i gives the plan's row count and the
// word offsets of its input indices, output indices and coefficient rows, each
// padded as the row-load idioms above expect.  On entering a unit of another
// object the wave takes, after the descriptor, its plan index, the plan's
// record (one scalar load each) and its input indices (one s_load_dwordx16), and recomputes the K
// input bases from them.
//
// The software pipeline keeps two tiles live, the one being stored and the
// one being loaded, and after advance() they may belong to objects with
// different plans: a PlannedTileOut therefore carries its OWN tile's
// coefficient and output-index offsets and row count, fixed when the tile's
// loads are issued, and the store of the earlier tile never reads the walk's
// current plan (`pl`).

struct PlannedTileOut {
  uint32_t* ob;
  uint64_t shard;
  uint32_t nvec, g0;
  uint32_t coeff_off, out_off, rows;  // the tile's own plan
};

// ragged_tails with each item's plan read through its descriptor.
template <int K>
__device__ __forceinline__ void planned_tails(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                              const Desc* __restrict__ descs, const Tail* __restrict__ tails,
                                              uint64_t ntails, const uint32_t* __restrict__ tab, uint32_t k) {
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t nthr = (uint64_t)gridDim.x * kBlock;
  for (uint64_t t = tid; t < ntails; t += nthr) {
    const Tail it = tails[t];
    const Desc* const d = descs + it.obj;
    const uint32_t* const r = tab + (uint64_t)d->reserved[0] * planset::kRecordWords;
    apply::apply_column<K>(in + d->src_off, out + d->dst_off, tab + r[3], tab + r[1], d->src_shard, tab + r[2],
                           d->dst_shard, r[0], k, (uint64_t)it.col);
  }
}

template <int K, int U, int C, int NC, bool NTL, bool NTS, bool DYN, bool PIPE>
__global__ __launch_bounds__(kBlock) void rs_apply_planned_kernel(
    const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const Desc* __restrict__ descs,
    const Unit* __restrict__ units, const Tail* __restrict__ tails, const uint32_t* __restrict__ tab, uint32_t nunits,
    uint64_t ntails, uint32_t k, uint32_t* __restrict__ ticket) {
  static_assert(K > 0 && K <= 16 && NC > 0 && NC <= 64, "compile-time k only");
  static_assert(PIPE || !DYN, "the dynamic walk is double-buffered");
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  UnitWalk<C, NC, DYN> w(ticket, units, descs, nunits, lane, wave, gridDim.x * kWaves);
  const uint32_t* sb[K];
  PlanRef pl{};  // the plan of the walk's current object
  auto bases = [&]() {
    pl = load_plan(tab, descs, w.obj);
    const u32x16 idx = *reinterpret_cast<const u32x16*>(tab + pl.in_off);  // K <= 16: one line
#pragma unroll
    for (int j = 0; j < K; ++j) sb[j] = in + w.d.src_off + (uint64_t)idx[j] * w.d.src_shard;
  };
  auto here = [&]() {
    return PlannedTileOut{out + w.d.dst_off, w.d.dst_shard, w.d.nvec, w.tile() * (64 * U) + lane,
                          pl.coeff_off,      pl.out_off,    pl.rows};
  };
  auto store = [&](const uint4(&x)[U][K], const PlannedTileOut& t) {
    apply::store_tile<K, U, NTS>(x, t.ob, tab + t.coeff_off, tab + t.out_off, t.shard, t.rows, t.g0, t.nvec);
  };
  if constexpr (PIPE) {
    if (w.live) {
      uint4 xa[U][K], xb[U][K];
      bases();
      PlannedTileOut ta = here(), tb = ta;
      apply::load_tile<K, U, NTL>(xa, sb, ta.g0, ta.nvec);
      for (;;) {
        w.advance();
        // Past the last unit the prefetch re-reads the current tile (unconditional loads, see load_tile).
        tb = ta;
        if (w.live) {
          if (w.fresh) bases();
          tb = here();
        }
        apply::load_tile<K, U, NTL>(xb, sb, tb.g0, tb.nvec);
        store(xa, ta);  // ta's own plan: bases() may just have moved `pl` on to tb's
        if (!w.live) break;
        w.advance();
        ta = tb;
        if (w.live) {
          if (w.fresh) bases();
          ta = here();
        }
        apply::load_tile<K, U, NTL>(xa, sb, ta.g0, ta.nvec);
        store(xb, tb);
        if (!w.live) break;
      }
    }
  } else {
    while (w.live) {
      uint4 x[U][K];
      if (w.fresh) bases();
      const PlannedTileOut t = here();
      apply::load_tile<K, U, NTL>(x, sb, t.g0, t.nvec);
      store(x, t);
      w.advance();
    }
  }
  w.finish();
  planned_tails<K>(in, out, descs, tails, ntails, tab, k);
}

// One column per lane over the same unit list (static walk), each unit with
// its object's plan: generic k through wide_dot, any alignment.
__global__ __launch_bounds__(kBlock) void rs_apply_planned_column_kernel(
    const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const Desc* __restrict__ descs,
    const Unit* __restrict__ units, const Tail* __restrict__ tails, const uint32_t* __restrict__ tab, uint32_t nunits,
    uint64_t ntails, uint32_t k, uint32_t tile_cols, uint32_t unit_tiles) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * kWaves;
  for (uint64_t e = wave; e < nunits; e += nwaves) {
    const Unit u = units[e];
    const ObjRef d = load_desc(descs, u.obj);
    const PlanRef pl = load_plan(tab, descs, u.obj);
    const uint32_t t1 = d.ntiles - u.tile < unit_tiles ? d.ntiles : u.tile + unit_tiles;
    const uint64_t b0 = (uint64_t)u.tile * tile_cols, bmax = (uint64_t)d.nvec << 2;
    const uint64_t b1 = (uint64_t)t1 * tile_cols < bmax ? (uint64_t)t1 * tile_cols : bmax;
    for (uint64_t b = b0 + lane; b < b1; b += 64)
      apply::apply_column<0>(in + d.src_off, out + d.dst_off, tab + pl.coeff_off, tab + pl.in_off, d.src_shard,
                             tab + pl.out_off, d.dst_shard, pl.rows, k, b);
  }
  planned_tails<0>(in, out, descs, tails, ntails, tab, k);
}

}  // namespace ragged

namespace {

using apply::kBlock;
constexpr bool kNtLoads = true;
constexpr bool kNtStores = true;

#define SLIME_RAGGED_ARGS(a)                                                                                  \
  (a).in, (a).out, (a).w.desc, (a).w.units, (a).w.tails, (a).p.coeff, (a).p.in_idx, (a).p.out_idx, (a).w.nunits, \
      (a).w.ntails, (a).p.rows, (a).w.k
#define SLIME_PLANNED_ARGS(a) \
  (a).in, (a).out, (a).w.desc, (a).w.units, (a).w.tails, (a).p.table, (a).w.nunits, (a).w.ntails, (a).w.k

template <int K, bool SET>
hipError_t launch_vectors(const RaggedLaunch& a, hipStream_t s) {
  constexpr int U = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K);
  // The static forms take the static pipelined apply launch's block budget (rs_apply.hip, pipe_blocks).
  return ragged::launch_scheduled(
      s, a.w.nunits, a.w.ntails, K <= 12 ? 256 : 1024, [&](auto dyn, auto pipe, uint64_t blocks, uint32_t* set) {
        constexpr bool DYN = decltype(dyn)::value, PIPE = decltype(pipe)::value;
        if constexpr (SET)
          hipLaunchKernelGGL((ragged::rs_apply_planned_kernel<K, U, C, kQueueCounters, kNtLoads, kNtStores, DYN, PIPE>),
                             dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_PLANNED_ARGS(a), set);
        else
          hipLaunchKernelGGL((ragged::rs_apply_ragged_kernel<K, U, C, kQueueCounters, kNtLoads, kNtStores, DYN, PIPE>),
                             dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_RAGGED_ARGS(a), set);
        return hipGetLastError();
      });
}

hipError_t launch_columns(const RaggedLaunch& a, hipStream_t s) {
  const uint64_t blocks = ragged::ragged_blocks(1024, a.w.nunits, a.w.ntails);
  if (a.p.table)
    hipLaunchKernelGGL(ragged::rs_apply_planned_column_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                       SLIME_PLANNED_ARGS(a), 256u * (uint32_t)a.w.U, (uint32_t)a.w.C);
  else
    hipLaunchKernelGGL(ragged::rs_apply_ragged_column_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                       SLIME_RAGGED_ARGS(a), 256u * (uint32_t)a.w.U, (uint32_t)a.w.C);
  return hipGetLastError();
}

#undef SLIME_RAGGED_ARGS
#undef SLIME_PLANNED_ARGS

}  // namespace

hipError_t launch_apply_ragged(const RaggedLaunch& a, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (a.w.nunits == 0 && a.w.ntails == 0) return hipSuccess;
  const bool set = a.p.table != nullptr;
  if (!set && a.p.rows == 0) return hipSuccess;
  if (a.w.k > 16 || !a.w.vec_ok) return launch_columns(a, s);
  // The vector kernels are instantiated with the geometry of their K: the tables must be cut by it.
  if (a.w.U != ragged::unroll_for_k((int)a.w.k) || a.w.C != ragged::unit_tiles_for_k((int)a.w.k))
    return hipErrorInvalidValue;
  return ragged::with_k(a.w.k, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    return set ? launch_vectors<K, true>(a, s) : launch_vectors<K, false>(a, s);
  });
}

}  // namespace slime
