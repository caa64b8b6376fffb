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
// Plan sets (slime_rs_planset_execute_batch): SET = true instantiates the two
// kernels with a plan PER OBJECT, named by the object's descriptor and read
// from a plan set's table (planset_table.hpp), as rs_bytes_ragged.hip's decode
// kernels do: one parameter list, `coeff` carrying the table under SET.  The
// SET = false instantiations compile to the bytes of the kernels that had no
// such parameter; two wordings decide that, both noted where they stand (the
// tile record and the unit go to their helpers by value).
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "planset_table.hpp"
#include "rs_apply_kernel.hpp"
#include "rs_ragged_launch.hpp"  // the grid, with_k and the choice between the schedules
#include "rs_ragged_walk.hpp"    // UnitWalk, load_desc, load_plan: shared with rs_verify_ragged.hip

namespace slime {
namespace ragged {

// coeff: the plan's rows, or (SET) the set's table; in_idx / out_idx / rows: the plan's (unused by SET).
#define SLIME_RAGGED_PARAMS                                                                                   \
  const uint32_t *__restrict__ in, uint32_t *__restrict__ out, const Desc *__restrict__ descs,                \
      const Unit *__restrict__ units, const Tail *__restrict__ tails, const uint32_t *__restrict__ coeff,     \
      const uint32_t *__restrict__ in_idx, const uint32_t *__restrict__ out_idx, uint32_t nunits,             \
      uint64_t ntails, uint32_t rows, uint32_t k

// Where a loaded tile goes: its object's output base and stride, the
// object's vector count and the lane's first vector -- and, under SET, the
// tile's OWN plan (offsets into the set's table and the row count), fixed when
// the tile's loads are issued.  The pipeline keeps two tiles live, and after
// advance() they may belong to objects with different plans: the store of the
// earlier tile reads its record, never the walk's current plan (`pl`).
template <bool SET>
struct TileOut {
  uint32_t* ob;
  uint64_t shard;
  uint32_t nvec, g0;
};
template <>
struct TileOut<true> : TileOut<false> {
  uint32_t coeff_off, out_off, rows;
};

// A loaded tile's rows to its object: with the launch's plan, or (SET) the
// tile's own, whatever the walk has moved on to.  The record goes by value: by
// reference the pipelined single-plan kernels compile to other bytes.
template <int K, int U, bool NTS, bool SET>
__device__ __forceinline__ void store_tile(const uint4 (&x)[U][K], const TileOut<SET> t, const uint32_t* coeff,
                                           const uint32_t* out_idx, uint32_t rows) {
  if constexpr (SET)
    apply::store_tile<K, U, NTS>(x, t.ob, coeff + t.coeff_off, coeff + t.out_off, t.shard, t.rows, t.g0, t.nvec);
  else
    apply::store_tile<K, U, NTS>(x, t.ob, coeff, out_idx, t.shard, rows, t.g0, t.nvec);
}

// The {object, column} items past the objects' last whole vectors, strided
// over the grid, one per lane (K == 0: generic k); under SET each item's plan
// is read through its descriptor.
template <int K, bool SET>
__device__ __forceinline__ void ragged_tails(SLIME_RAGGED_PARAMS) {
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t nthr = (uint64_t)gridDim.x * kBlock;
  for (uint64_t t = tid; t < ntails; t += nthr) {
    const Tail it = tails[t];
    const Desc* const d = descs + it.obj;
    PlanRows pl{coeff, out_idx, rows};
    const uint32_t* ii = in_idx;
    if constexpr (SET) {
      const PlanRef p = read_plan(coeff, d);
      pl = whole_plan(coeff, p);
      ii = coeff + p.in_off;
    }
    apply::apply_column<K>(in + d->src_off, out + d->dst_off, pl.coeff, ii, d->src_shard, pl.oidx, d->dst_shard,
                           pl.rows, k, (uint64_t)it.col);
  }
}

// SET: every object its own plan (slime_rs_planset_execute_batch).  The
// batch's descriptors carry a plan index (Desc::reserved[0]) into the set's
// table (planset_table.hpp): the 64-byte record of plan i at word 16 i gives
// the plan's row count and the word offsets of its input indices, output
// indices and coefficient rows, each padded as the row-load idioms expect.  On
// entering a unit of another object the wave takes, after the descriptor, its
// plan index, the plan's record (one scalar load each) and its input indices
// (one s_load_dwordx16), and recomputes the K input bases from them.
template <int K, int U, int C, int NC, bool NTL, bool NTS, bool DYN, bool PIPE, bool SET>
__global__ __launch_bounds__(kBlock) void rs_apply_ragged_kernel(SLIME_RAGGED_PARAMS,
                                                                 uint32_t* __restrict__ ticket) {
  static_assert(K > 0 && K <= 16 && NC > 0 && NC <= 64, "compile-time k only");
  static_assert(PIPE || !DYN, "the dynamic walk is double-buffered");
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  UnitWalk<C, NC, DYN> w(ticket, units, descs, nunits, lane, wave, gridDim.x * kWaves);
  const uint32_t* sb[K];
  PlanRef pl{};  // SET: the plan of the walk's current object
  auto bases = [&]() {
    if constexpr (SET) {
      pl = load_plan(coeff, descs, w.obj);
      const u32x16 idx = *reinterpret_cast<const u32x16*>(coeff + pl.in_off);  // K <= 16: one line
#pragma unroll
      for (int j = 0; j < K; ++j) sb[j] = in + w.d.src_off + (uint64_t)idx[j] * w.d.src_shard;
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) sb[j] = in + w.d.src_off + (uint64_t)in_idx[j] * w.d.src_shard;
    }
  };
  auto here = [&]() {
    const TileOut<false> t{out + w.d.dst_off, w.d.dst_shard, w.d.nvec, w.tile() * (64 * U) + lane};
    if constexpr (SET)
      return TileOut<true>{t, pl.coeff_off, pl.out_off, pl.rows};
    else
      return t;
  };
  if constexpr (PIPE) {
    if (w.live) {
      uint4 xa[U][K], xb[U][K];
      bases();
      TileOut<SET> ta = here(), tb = ta;
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
        // ta's own plan: bases() may just have moved `pl` on to tb's
        store_tile<K, U, NTS>(xa, ta, coeff, out_idx, rows);
        if (!w.live) break;
        w.advance();
        ta = tb;
        if (w.live) {
          if (w.fresh) bases();
          ta = here();
        }
        apply::load_tile<K, U, NTL>(xa, sb, ta.g0, ta.nvec);
        store_tile<K, U, NTS>(xb, tb, coeff, out_idx, rows);
        if (!w.live) break;
      }
    }
  } else {
    while (w.live) {
      uint4 x[U][K];
      if (w.fresh) bases();
      const TileOut<SET> t = here();
      apply::load_tile<K, U, NTL>(x, sb, t.g0, t.nvec);
      store_tile<K, U, NTS>(x, t, coeff, out_idx, rows);
      w.advance();
    }
  }
  w.finish();
  ragged_tails<K, SET>(in, out, descs, units, tails, coeff, in_idx, out_idx, nunits, ntails, rows, k);
}

// One column per lane over the same unit list (static walk): generic k
// through wide_dot, any alignment; under SET each unit with its object's
// plan.  tile_cols = 256 U, unit_tiles = C of the batch's geometry.
template <bool SET>
__global__ __launch_bounds__(kBlock) void rs_apply_ragged_column_kernel(SLIME_RAGGED_PARAMS, uint32_t tile_cols,
                                                                        uint32_t unit_tiles) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * kWaves;
  for (uint64_t e = wave; e < nunits; e += nwaves) {
    const Unit u = units[e];
    const ObjRef d = load_desc(descs, u.obj);
    PlanRows pl{coeff, out_idx, rows};
    const uint32_t* ii = in_idx;
    if constexpr (SET) {
      const PlanRef p = load_plan(coeff, descs, u.obj);
      pl = whole_plan(coeff, p);
      ii = coeff + p.in_off;
    }
    const ColRange c = unit_columns(d.ntiles, u, tile_cols, unit_tiles, d.nvec);
    for (uint64_t b = c.b0 + lane; b < c.b1; b += 64)
      apply::apply_column<0>(in + d.src_off, out + d.dst_off, pl.coeff, ii, d.src_shard, pl.oidx, d.dst_shard, pl.rows,
                             k, b);
  }
  ragged_tails<0, SET>(in, out, descs, units, tails, coeff, in_idx, out_idx, nunits, ntails, rows, k);
}

#undef SLIME_RAGGED_PARAMS

}  // namespace ragged

namespace {

using apply::kBlock;
constexpr bool kNtLoads = true;
constexpr bool kNtStores = true;

#define SLIME_RAGGED_ARGS(a, SET)                                                                        \
  (a).in, (a).out, (a).w.desc, (a).w.units, (a).w.tails, (SET) ? (a).p.table : (a).p.coeff, (a).p.in_idx, \
      (a).p.out_idx, (a).w.nunits, (a).w.ntails, (a).p.rows, (a).w.k

template <int K, bool SET>
hipError_t launch_vectors(const RaggedLaunch& a, hipStream_t s) {
  constexpr int U = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K);
  // The static forms take the static pipelined apply launch's block budget (rs_apply.hip, pipe_blocks).
  return ragged::launch_scheduled(
      s, a.w.nunits, a.w.ntails, K <= 12 ? 256 : 1024, [&](auto dyn, auto pipe, uint64_t blocks, uint32_t* set) {
        constexpr bool DYN = decltype(dyn)::value, PIPE = decltype(pipe)::value;
        hipLaunchKernelGGL(
            (ragged::rs_apply_ragged_kernel<K, U, C, kQueueCounters, kNtLoads, kNtStores, DYN, PIPE, SET>),
            dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_RAGGED_ARGS(a, SET), set);
        return hipGetLastError();
      });
}

template <bool SET>
hipError_t launch_columns(const RaggedLaunch& a, hipStream_t s) {
  const uint64_t blocks = ragged::ragged_blocks(1024, a.w.nunits, a.w.ntails);
  hipLaunchKernelGGL(ragged::rs_apply_ragged_column_kernel<SET>, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                     SLIME_RAGGED_ARGS(a, SET), 256u * (uint32_t)a.w.U, (uint32_t)a.w.C);
  return hipGetLastError();
}

#undef SLIME_RAGGED_ARGS

}  // namespace

hipError_t launch_apply_ragged(const RaggedLaunch& a, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (a.w.nunits == 0 && a.w.ntails == 0) return hipSuccess;
  const bool set = a.p.table != nullptr;
  if (!set && a.p.rows == 0) return hipSuccess;
  if (a.w.k > 16 || !a.w.vec_ok) return set ? launch_columns<true>(a, s) : launch_columns<false>(a, s);
  // The vector kernels are instantiated with the geometry of their K: the tables must be cut by it.
  if (a.w.U != ragged::unroll_for_k((int)a.w.k) || a.w.C != ragged::unit_tiles_for_k((int)a.w.k))
    return hipErrorInvalidValue;
  return ragged::with_k(a.w.k, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    return set ? launch_vectors<K, true>(a, s) : launch_vectors<K, false>(a, s);
  });
}

}  // namespace slime
