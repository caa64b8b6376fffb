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
// verify's StepRef therefore carry their own tile's mapping, plan rows and output
// base, fixed when the tile's loads are issued; the store or compare of the
// earlier tile never reads the walk's current object (`cur`, `cur_m`).
//
// Tails: the {object, column} items past the objects' last whole vectors are
// strided over the grid after the walk, one per lane, each with its own
// object's mapping (and plan).
//
// Verify: the kernels' bodies are rs_verify_ragged.hip's (BYTES;
// rs_verify_ragged_kernel.hpp, rs_verify_ragged_walk_body.hpp), entered here
// with the mapping argument.  A launch tallies at most 64 rows; the host
// launches row blocks of 64 as rs_verify_ragged.hip does.  Only plain C++
// vector stores and vector atomics write memory.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "planset_table.hpp"
#include "rs_apply_kernel.hpp"
#include "rs_bytes_kernel.hpp"  // load_raw_tile, rows_tile, be
#include "rs_ragged_launch.hpp"
#include "rs_ragged_walk.hpp"
#include "rs_verify_ragged_kernel.hpp"  // the verify kernels' bodies: shared with rs_verify_ragged.hip
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
using ragged::PlanRows;
using ragged::Tail;
using ragged::Unit;
using ragged::UnitWalk;

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
    if constexpr (SET) {
      const PlanRef p = ragged::read_plan(coeff, d);
      pl = ragged::whole_plan(coeff, p);
      ii = coeff + p.in_off;
    }
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
      cur = ragged::whole_plan(coeff, pl);
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
      pl = ragged::whole_plan(coeff, p);
      ii = coeff + p.in_off;
    }
    const uint32_t m = mapping[u.obj];
    const ragged::ColRange c = ragged::unit_columns(d.ntiles, u, tile_cols, unit_tiles, d.nvec);
    for (uint64_t b = c.b0 + lane; b < c.b1; b += 64)
      decode_column<0>(in + (d.src_off << 2), out + (d.dst_off << 2), pl.coeff, ii, d.src_shard << 2, pl.oidx,
                       d.dst_shard << 2, pl.rows, k, m, b << 2);
  }
  decode_tails<0, SET>(in, out, descs, units, tails, coeff, in_idx, out_idx, mapping, nunits, ntails, rows, k);
}

#undef SLIME_BDECODE_PARAMS

// ---- verify: the byte forms' entry points of rs_verify_ragged_kernel.hpp's bodies --------

template <int K, int W, int R, int UB, int C, int NC, bool DYN, bool PIPE, bool SET>
__global__ __launch_bounds__(kBlock) void rs_verify_bytes_ragged_kernel(SLIME_RVERIFY_PARAMS,
                                                                        uint32_t* __restrict__ ticket) {
  using namespace verify;
  constexpr bool BYTES = true;
#include "rs_verify_ragged_walk_body.hpp"
}

template <bool SET>
__global__ __launch_bounds__(kBlock) void rs_verify_bytes_ragged_column_kernel(SLIME_RVERIFY_PARAMS,
                                                                               uint32_t tile_cols,
                                                                               uint32_t unit_tiles) {
  verify::verify_ragged_columns<SET, true>(SLIME_RVERIFY_PASS, tile_cols, unit_tiles);
}

}  // namespace bytes_ragged

namespace {

using apply::kBlock;

// ---- decode launches: the grids are launch_apply_ragged's (rs_ragged.hip) ----

#define SLIME_BDECODE_ARGS(a, SET)                                                                            \
  (a).in, (a).out, (a).w.desc, (a).w.units, (a).w.tails, (SET) ? (a).p.table : (a).p.coeff, (a).p.in_idx,      \
      (a).p.out_idx, (a).mapping, (a).w.nunits, (a).w.ntails, (a).p.rows, (a).w.k

template <int K, bool SET>
hipError_t decode_vectors(const RaggedBytesLaunch& a, hipStream_t s) {
  constexpr int U = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K);
  return ragged::launch_scheduled(
      s, a.w.nunits, a.w.ntails, K <= 12 ? 256 : 1024, [&](auto dyn, auto pipe, uint64_t blocks, uint32_t* set) {
        constexpr bool DYN = decltype(dyn)::value, PIPE = decltype(pipe)::value;
        hipLaunchKernelGGL((bytes_ragged::rs_decode_ragged_kernel<K, U, C, kQueueCounters, DYN, PIPE, SET>),
                           dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_BDECODE_ARGS(a, SET), set);
        return hipGetLastError();
      });
}

template <bool SET>
hipError_t decode_columns(const RaggedBytesLaunch& a, hipStream_t s) {
  const uint64_t blocks = ragged::ragged_blocks(1024, a.w.nunits, a.w.ntails);
  hipLaunchKernelGGL(bytes_ragged::rs_decode_ragged_column_kernel<SET>, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                     SLIME_BDECODE_ARGS(a, SET), 256u * (uint32_t)a.w.U, (uint32_t)a.w.C);
  return hipGetLastError();
}

#undef SLIME_BDECODE_ARGS

// ---- verify launches: launch_verify_ragged's (rs_verify_ragged.hip) ----

using RowBlock = ragged::RowBlock<RaggedBytesVerifyLaunch>;

#define SLIME_BVERIFY_ARGS(b, SET)                                                                                 \
  (b).v.in, (b).v.cmp, (b).v.w.desc, (b).v.w.units, (b).v.w.tails,                                                 \
      (SET) ? (b).v.p.table : (b).v.p.coeff + (uint64_t)(b).r0 * coeff_stride((b).v.w.k), (b).v.p.in_idx,         \
      (SET) ? (const uint32_t*)nullptr : (b).v.p.out_idx + (b).r0, (b).v.mapping,                                  \
      (unsigned long long*)(b).v.mismatches + (b).r0, (unsigned long long*)(b).v.first + (b).r0, (b).v.w.nunits,   \
      (b).v.w.ntails, (SET) ? 0u : (b).rows_c, (b).v.w.k, (SET) ? (b).r0 : 0u, (b).v.p.rows

template <int K, int R, bool SET>
hipError_t verify_vectors(const RowBlock& b, hipStream_t s) {
  constexpr int UB = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K), W = verify_step::width(K, R);
  // Static forms: fat waves one block a CU, thin ones (one vector a lane) four, as the uniform verify launch.
  return ragged::launch_scheduled(
      s, b.v.w.nunits, b.v.w.ntails, W == 1 ? 1024 : 256, [&](auto dyn, auto pipe, uint64_t blocks, uint32_t* set) {
        constexpr bool DYN = decltype(dyn)::value, PIPE = decltype(pipe)::value;
        hipLaunchKernelGGL((bytes_ragged::rs_verify_bytes_ragged_kernel<K, W, R, UB, C, kQueueCounters, DYN, PIPE, SET>),
                           dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_BVERIFY_ARGS(b, SET), set);
        return hipGetLastError();
      });
}

template <int K>
hipError_t verify_rows(const RowBlock& b, hipStream_t s) {
  const bool set = b.v.p.table != nullptr;
  if (verify_step::stored_rows(b.rows_c) == 2)
    return set ? verify_vectors<K, 2, true>(b, s) : verify_vectors<K, 2, false>(b, s);
  return set ? verify_vectors<K, 4, true>(b, s) : verify_vectors<K, 4, false>(b, s);
}

hipError_t verify_columns(const RowBlock& b, hipStream_t s) {
  const uint64_t blocks = ragged::ragged_blocks(1024, b.v.w.nunits, b.v.w.ntails);
  if (b.v.p.table)
    hipLaunchKernelGGL(bytes_ragged::rs_verify_bytes_ragged_column_kernel<true>, dim3((uint32_t)blocks), dim3(kBlock),
                       0, s, SLIME_BVERIFY_ARGS(b, true), 256u * (uint32_t)b.v.w.U, (uint32_t)b.v.w.C);
  else
    hipLaunchKernelGGL(bytes_ragged::rs_verify_bytes_ragged_column_kernel<false>, dim3((uint32_t)blocks),
                       dim3(kBlock), 0, s, SLIME_BVERIFY_ARGS(b, false), 256u * (uint32_t)b.v.w.U, (uint32_t)b.v.w.C);
  return hipGetLastError();
}

#undef SLIME_BVERIFY_ARGS

}  // namespace

hipError_t launch_decode_bytes_ragged(const RaggedBytesLaunch& a, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (a.w.nunits == 0 && a.w.ntails == 0) return hipSuccess;
  const bool set = a.p.table != nullptr;
  if (!set && a.p.rows == 0) return hipSuccess;
  if (a.w.k > 16 || !a.w.vec_ok) return set ? decode_columns<true>(a, s) : decode_columns<false>(a, s);
  // The vector kernels are instantiated with the geometry of their K: the tables must be cut by it.
  if (a.w.U != ragged::unroll_for_k((int)a.w.k) || a.w.C != ragged::unit_tiles_for_k((int)a.w.k))
    return hipErrorInvalidValue;
  return ragged::with_k(a.w.k, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    return set ? decode_vectors<K, true>(a, s) : decode_vectors<K, false>(a, s);
  });
}

hipError_t launch_verify_bytes_ragged(const RaggedBytesVerifyLaunch& v, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (v.w.nobj == 0 || v.p.rows == 0) return hipSuccess;
  if (hipError_t e = launch_verify_init(v.mismatches, v.first, v.w.nobj * v.p.rows, s)) return e;
  if (v.w.nunits == 0 && v.w.ntails == 0) return hipSuccess;  // an empty batch: nothing but the initialisation
  const bool vec = v.w.k <= 16 && v.w.vec_ok;
  if (vec && (v.w.U != ragged::unroll_for_k((int)v.w.k) || v.w.C != ragged::unit_tiles_for_k((int)v.w.k)))
    return hipErrorInvalidValue;
  return ragged::for_row_blocks(v, [&](const RowBlock& b) {
    if (!vec) return verify_columns(b, s);
    return ragged::with_k(v.w.k, [&](auto kc) { return verify_rows<decltype(kc)::value>(b, s); });
  });
}

}  // namespace slime
