// Ragged byte encode for CDNA4 (gfx950): slime_rs_encode_objects_batch and the
// re-encode of slime_rs_resolve_fallbacks_batch -- the fused byte encode
// (rs_bytes_kernel.hpp's header comment) over the objects of a ragged batch,
// each with its own size, padding, data-chunk tail and MapToGF mapping.
//
// A call is a linear chain of kernels on the stream:
//   init      mapping[o] = 0, status[o] = 0
//   pass 0    every object with work encoded with m = 0; MapToGF's two flag
//             bits (bytes::flag_bits) OR-ed into status[o]
//   select    flags -> mapping[o] and status[o]: 1 (random fallback), 0 (final)
//             or kPending, the transient mark of an object to re-encode
//   pass 1    the pending objects again with m = mapping[o]; a unit of any
//             other object is passed over before any load
//   clear     kPending -> 0
// slime_rs_resolve_fallbacks_batch marks the objects it found a mapping for
// kPending itself and runs pass 1 and clear.  Whole objects are re-encoded:
// no mid-object switch, redo list or top-bit correction.
//
// A pass is one kernel with two steps:
//   walk   rs_decode_ragged_kernel's loop (rs_bytes_ragged.hip) -- UnitWalk, the
//          U and C of the batch's k, the dynamic, static double-buffered and
//          static one-tile walks, chosen as launch_decode_bytes_ragged chooses
//          -- over the object's INTERIOR vectors only (encode_edge.hpp): tiles
//          at or past the bound are passed over before their loads, stores are
//          clipped to it.  No word there is partial or padding, so the
//          consumer is decode's plus the flag folding.
//   edge   the columns from the bound to L - 1 -- at most k + 3 an object, the
//          L % 4 columns of the tail list among them -- one {object, column}
//          a lane, strided over the grid by object index (never over a list
//          that grows with the batch): packed_word's checks, the data-chunk
//          tail rewritten in src, flags from the words below nw only.
// k > 16, or a base that is not 4-byte aligned: the walk runs one column a lane
// through apply::wide_dot over the same unit list (static), like its siblings.
//
// The flags belong to the TILE's object (§18's rule for the mapping, applied
// again): the pipeline consumes a tile after the walk has moved on, so EncTile
// carries its object.  A wave folds the byte-swapped raw words of the tiles it
// consumes into running maxima (bytes::Flags) while they stay in one object,
// and does one ballot and one atomicOr when the consumed tile's object changes
// and once after the walk -- never an atomic per tile.  Lanes past the clipped
// end re-read the object's last interior vector, which changes no maximum.
//
// Only plain C++ vector stores and vector atomics write memory.
#include <hip/hip_runtime.h>

#include "encode_edge.hpp"
#include "kernels.hpp"
#include "rs_apply_kernel.hpp"
#include "rs_bytes_kernel.hpp"  // load_raw_tile, rows_tile, be, Flags, packed_word
#include "rs_ragged_launch.hpp"
#include "rs_ragged_walk.hpp"

namespace slime {
namespace bytes_ragged_encode {

using apply::kBlock;
using apply::kWaves;
using bytes::be;
using bytes::Flags;
using ragged::Desc;
using ragged::ObjRef;
using ragged::Unit;
using ragged::UnitWalk;

constexpr uint32_t kPending = kRaggedEncodePending;

#define SLIME_BENCODE_PARAMS                                                                                  \
  uint8_t *in, uint8_t *out, const Desc *__restrict__ descs, const Unit *__restrict__ units,                  \
      const uint32_t *__restrict__ coeff, const uint32_t *__restrict__ out_idx,                               \
      const uint64_t *__restrict__ sizes, const uint32_t *mapping, uint32_t *status, uint32_t nunits,         \
      uint32_t nobj, uint32_t rows, uint32_t k, uint32_t pass

// A wave's flag bits of object obj: one ballot pair, one atomic from lane 0.
__device__ __forceinline__ void or_wave_flags(uint32_t* status, uint32_t obj, uint32_t f, uint32_t lane) {
  const uint64_t a1 = __ballot(f & 1u), a2 = __ballot(f & 2u);
  const uint32_t wf = (a1 ? 1u : 0u) | (a2 ? 2u : 0u);
  if (wf && lane == 0) atomicOr(status + obj, wf);
}

// One column (byte offset 4 col into every chunk) of one object with every
// check: padding, the partial word, the data-chunk tail rewritten in src, the
// parity rows.  Returns the flag bits of the column's words below nw.
// K > 0: compile-time k, the symbols held in registers; K == 0: generic k.
template <int K>
__device__ __forceinline__ uint32_t encode_column(uint8_t* ib, uint8_t* ob, const uint32_t* __restrict__ coeff,
                                                  uint64_t in_shard, const uint32_t* __restrict__ out_idx,
                                                  uint64_t out_shard, uint32_t rows, uint32_t k, uint32_t m,
                                                  uint64_t L, uint64_t col, const edge::Geom& g) {
  const bytes::ObjWords ow{g.nw, g.tailmask};
  const uint64_t off = col << 2;
  uint32_t bits = 0;
  uint32_t x[K > 0 ? K : 1];
  // Data chunk j's word of this column: flags, the tail rewrite, the symbol.
  auto take = [&](uint32_t j) {
    uint32_t* const p = reinterpret_cast<uint32_t*>(ib + (uint64_t)j * in_shard + off);
    const uint64_t w = (uint64_t)j * L + col;
    bool pad;
    const uint32_t packed = bytes::packed_word(*p, w, ow, &pad);
    if (!pad) bits |= bytes::flag_bits(packed);
    if (w + 1 >= ow.nw) *p = be(pad ? m : packed);  // fix_data_tail_one, one column
    return pad ? 0u : packed ^ m;
  };
  if constexpr (K > 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) x[j] = take(j);
  } else {
    for (uint32_t j = 0; j < k; ++j) (void)take(j);
  }
  // Generic k: the symbols are read again from the rewritten chunks (the
  // rewrite keeps a partial word's packed value, and padding is symbol 0
  // whatever its bytes).
  auto again = [&](uint32_t j) {
    bool pad;
    const uint32_t packed = bytes::packed_word(*reinterpret_cast<const uint32_t*>(ib + (uint64_t)j * in_shard + off),
                                               (uint64_t)j * L + col, ow, &pad);
    return pad ? 0u : packed ^ m;
  };
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
      r = apply::wide_dot(coeff + (uint64_t)i * apply::wide_coeff_stride(k), k, again);
    }
    *reinterpret_cast<uint32_t*>(ob + (uint64_t)out_idx[i] * out_shard + off) = be(r ^ m);
  }
  return bits;
}

// The edge step: item t is column 4 interior + t % (k + 3) of object
// t / (k + 3), one item a lane over the grid.
template <int K>
__device__ __forceinline__ void encode_edges(SLIME_BENCODE_PARAMS) {
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t nthr = (uint64_t)gridDim.x * kBlock;
  const uint32_t ec = edge::edge_columns_max(k);
  for (uint64_t t = tid; t < (uint64_t)nobj * ec; t += nthr) {
    const uint32_t obj = (uint32_t)(t / ec);
    const Desc* const d = descs + obj;
    const uint64_t L = d->ncols;
    if (L == 0) continue;  // no work: its size is not read
    if (pass && status[obj] != kPending) continue;
    const edge::Geom g = edge::geom(sizes[obj], L, k);
    const uint64_t col = ((uint64_t)g.interior << 2) + t % ec;
    if (col >= L) continue;
    const uint32_t m = pass ? mapping[obj] : 0u;
    const uint32_t bits = encode_column<K>(in + (d->src_off << 2), out + (d->dst_off << 2), coeff, d->src_shard << 2,
                                           out_idx, d->dst_shard << 2, rows, k, m, L, col, g);
    if (!pass && bits) atomicOr(status + obj, bits);
  }
}

// Where a loaded tile goes and how it is read: its object (for the flags),
// output base and chunk stride (bytes), the object's interior vector count,
// the tile's first vector, and the mapping it is encoded with.
struct EncTile {
  uint8_t* ob;
  uint64_t shard;
  uint32_t obj, nvec, t0, m;
};

template <int K, int U, int C, int NC, bool DYN, bool PIPE>
__global__ __launch_bounds__(kBlock) void rs_encode_ragged_kernel(SLIME_BENCODE_PARAMS, uint32_t* __restrict__ ticket) {
  static_assert(K > 0 && K <= 16 && NC > 0 && NC <= 64, "compile-time k only");
  static_assert(PIPE || !DYN, "the dynamic walk is double-buffered");
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  UnitWalk<C, NC, DYN> w(ticket, units, descs, nunits, lane, wave, gridDim.x * kWaves);
  // The walk's current object: read when a tile's loads are issued, never by a consumer.
  // INVARIANT: sb always belongs to the object of the last tile returned by here().  The
  // prefetch past a wave's last tile re-reads that tile through sb, so sb must never move on
  // to an object whose tiles are only passed over: its chunks may be far shorter than the
  // offsets of the tile being re-read.
  const uint8_t* sb[K];
  uint32_t sb_obj = ~0u;
  uint32_t cur_m = 0, cur_nvec = 0;
  bool cur_skip = false;
  // What decides whether the object's tiles are loaded at all (wave-uniform scalar loads);
  // pass 1 reads the status first and nothing else of an object that is not pending.
  auto probe = [&]() {
    if (pass) {
      cur_skip = status[w.obj] != kPending;
      if (cur_skip) return;
      cur_m = mapping[w.obj];
    }
    cur_nvec = edge::geom(sizes[w.obj], descs[w.obj].ncols, K).interior;
  };
  // After the walk moved: tiles of an object that is not pending (pass 1) and tiles at or
  // past the interior bound are passed over before any load -- so a loaded tile has a vector
  // below its bound -- and only for a tile that will be loaded do the bases move to its object.
  auto settle = [&]() {
    while (w.live) {
      if (w.fresh) probe();
      if (!cur_skip && w.tile() * (64 * U) < cur_nvec) break;
      w.advance();
    }
    if (w.live && sb_obj != w.obj) {
      sb_obj = w.obj;
#pragma unroll
      for (int j = 0; j < K; ++j) sb[j] = in + ((w.d.src_off + (uint64_t)j * w.d.src_shard) << 2);
    }
  };
  auto here = [&]() {
    return EncTile{out + (w.d.dst_off << 2), w.d.dst_shard << 2, w.obj, cur_nvec, w.tile() * (64 * U), cur_m};
  };
  auto load = [&](uint4(&x)[U][K], const EncTile& t) { bytes::load_raw_tile<K, U>(x, sb, t.t0 + lane, t.nvec); };
  // The consumed tiles' flags, while they stay in one object.
  Flags fl;
  uint32_t fl_obj = ~0u;
  auto flush = [&]() {
    if (!pass && fl_obj != ~0u) or_wave_flags(status, fl_obj, fl.bits(), lane);
    fl = Flags{};
  };
  // The tile's OWN object and mapping (t), whatever the walk has moved on to.
  auto consume = [&](uint4(&x)[U][K], const EncTile& t) {
    if (t.obj != fl_obj) {
      flush();
      fl_obj = t.obj;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const uint32_t p0 = be(x[u][j].x), p1 = be(x[u][j].y), p2 = be(x[u][j].z), p3 = be(x[u][j].w);
        fl.add(0, p0), fl.add(1, p1), fl.add(2, p2), fl.add(3, p3);
        x[u][j] = make_uint4(p0 ^ t.m, p1 ^ t.m, p2 ^ t.m, p3 ^ t.m);
      }
    bytes::rows_tile<K, U>(x, rows, coeff, out_idx, t.ob, t.shard, t.t0 + lane, t.nvec, t.m);
  };
  settle();
  if constexpr (PIPE) {
    if (w.live) {
      uint4 xa[U][K], xb[U][K];
      EncTile ta = here(), tb = ta;
      load(xa, ta);
      for (;;) {
        w.advance();
        settle();
        // Past the last tile the prefetch re-reads the current one (unconditional loads, see load_raw_tile).
        tb = ta;
        if (w.live) tb = here();
        load(xb, tb);
        consume(xa, ta);  // ta's own object and mapping: settle() may just have moved the walk on to tb's
        if (!w.live) break;
        w.advance();
        settle();
        ta = tb;
        if (w.live) ta = here();
        load(xa, ta);
        consume(xb, tb);
        if (!w.live) break;
      }
    }
  } else {
    while (w.live) {
      uint4 x[U][K];
      const EncTile t = here();
      load(x, t);
      consume(x, t);
      w.advance();
      settle();
    }
  }
  flush();
  w.finish();
  encode_edges<K>(in, out, descs, units, coeff, out_idx, sizes, mapping, status, nunits, nobj, rows, k, pass);
}

// One column per lane over the same unit list (static walk): generic k
// through wide_dot, any alignment.  tile_cols = 256 U, unit_tiles = C of the
// batch's geometry.
__global__ __launch_bounds__(kBlock) void rs_encode_ragged_column_kernel(SLIME_BENCODE_PARAMS, uint32_t tile_cols,
                                                                         uint32_t unit_tiles) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * kWaves;
  for (uint64_t e = wave; e < nunits; e += nwaves) {
    const Unit u = units[e];
    if (pass && status[u.obj] != kPending) continue;
    const ObjRef d = ragged::load_desc(descs, u.obj);
    const uint64_t L = descs[u.obj].ncols;
    const edge::Geom g = edge::geom(sizes[u.obj], L, k);
    const uint32_t m = pass ? mapping[u.obj] : 0u;
    const ragged::ColRange c = ragged::unit_columns(d.ntiles, u, tile_cols, unit_tiles, g.interior);
    uint32_t bits = 0;
    for (uint64_t b = c.b0 + lane; b < c.b1; b += 64)
      bits |= encode_column<0>(in + (d.src_off << 2), out + (d.dst_off << 2), coeff, d.src_shard << 2, out_idx,
                               d.dst_shard << 2, rows, k, m, L, b, g);
    if (!pass) or_wave_flags(status, u.obj, bits, lane);
  }
  encode_edges<0>(in, out, descs, units, coeff, out_idx, sizes, mapping, status, nunits, nobj, rows, k, pass);
}

#undef SLIME_BENCODE_PARAMS

__global__ void encode_init_kernel(uint32_t* __restrict__ mapping, uint32_t* __restrict__ status, uint32_t nobj) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= nobj) return;
  mapping[o] = 0u;
  status[o] = 0u;
}

// select_mapping_kernel (rs_bytes.hip) with the pending mark: an object whose
// mapping is not 0 has parity from pass 0 that is not final.
__global__ void encode_select_kernel(uint32_t* __restrict__ mapping, uint32_t* __restrict__ status, uint32_t nobj) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= nobj) return;
  const uint32_t f = status[o];
  const bool zero_ok = !(f & 1u), high_ok = !(f & 2u);
  mapping[o] = zero_ok ? 0u : (high_ok ? 0x80000000u : 0u);
  status[o] = zero_ok ? 0u : (high_ok ? kPending : 1u);
}

__global__ void encode_clear_kernel(uint32_t* __restrict__ status, uint32_t nobj) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= nobj) return;
  if (status[o] == kPending) status[o] = 0u;
}

}  // namespace bytes_ragged_encode

namespace {

using apply::kBlock;

// The per-lane items of a pass are its edge columns, not the tail list.
uint64_t edge_items(const RaggedEncodeLaunch& a) { return a.w.nobj * edge::edge_columns_max(a.w.k); }

#define SLIME_BENCODE_ARGS(a, pass)                                                                              \
  (a).src, (a).dst, (a).w.desc, (a).w.units, (a).p.coeff, (a).p.out_idx, (a).sizes, (a).mapping, (a).status,      \
      (a).w.nunits, (uint32_t)(a).w.nobj, (a).p.rows, (a).w.k, (uint32_t)(pass)

// The grids are launch_decode_bytes_ragged's.
template <int K>
hipError_t pass_vectors(const RaggedEncodeLaunch& a, int pass, hipStream_t s) {
  constexpr int U = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K);
  return ragged::launch_scheduled(
      s, a.w.nunits, edge_items(a), K <= 12 ? 256 : 1024, [&](auto dyn, auto pipe, uint64_t blocks, uint32_t* set) {
        constexpr bool DYN = decltype(dyn)::value, PIPE = decltype(pipe)::value;
        hipLaunchKernelGGL((bytes_ragged_encode::rs_encode_ragged_kernel<K, U, C, kQueueCounters, DYN, PIPE>),
                           dim3((uint32_t)blocks), dim3(kBlock), 0, s, SLIME_BENCODE_ARGS(a, pass), set);
        return hipGetLastError();
      });
}

hipError_t pass_columns(const RaggedEncodeLaunch& a, int pass, hipStream_t s) {
  const uint64_t blocks = ragged::ragged_blocks(1024, a.w.nunits, edge_items(a));
  hipLaunchKernelGGL(bytes_ragged_encode::rs_encode_ragged_column_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s,
                     SLIME_BENCODE_ARGS(a, pass), 256u * (uint32_t)a.w.U, (uint32_t)a.w.C);
  return hipGetLastError();
}

#undef SLIME_BENCODE_ARGS

hipError_t encode_pass(const RaggedEncodeLaunch& a, int pass, hipStream_t s) {
  if (a.w.k > 16 || !a.w.vec_ok) return pass_columns(a, pass, s);
  // The vector kernels are instantiated with the geometry of their K: the tables must be cut by it.
  if (a.w.U != ragged::unroll_for_k((int)a.w.k) || a.w.C != ragged::unit_tiles_for_k((int)a.w.k))
    return hipErrorInvalidValue;
  return ragged::with_k(a.w.k, [&](auto kc) { return pass_vectors<decltype(kc)::value>(a, pass, s); });
}

}  // namespace

hipError_t launch_encode_bytes_ragged(const RaggedEncodeLaunch& a, RaggedEncodeStep step, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (a.w.nobj == 0) return hipSuccess;
  const uint32_t nobj = (uint32_t)a.w.nobj;
  const dim3 per_obj((nobj + 255) / 256);
  switch (step) {
    case RaggedEncodeStep::Init:
      hipLaunchKernelGGL(bytes_ragged_encode::encode_init_kernel, per_obj, dim3(256), 0, s, a.mapping, a.status, nobj);
      return hipGetLastError();
    case RaggedEncodeStep::Pass0: return a.has_work ? encode_pass(a, 0, s) : hipSuccess;
    case RaggedEncodeStep::Select:
      hipLaunchKernelGGL(bytes_ragged_encode::encode_select_kernel, per_obj, dim3(256), 0, s, a.mapping, a.status, nobj);
      return hipGetLastError();
    case RaggedEncodeStep::Pass1: return a.has_work ? encode_pass(a, 1, s) : hipSuccess;
    case RaggedEncodeStep::Clear:
      hipLaunchKernelGGL(bytes_ragged_encode::encode_clear_kernel, per_obj, dim3(256), 0, s, a.status, nobj);
      return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

}  // namespace slime
