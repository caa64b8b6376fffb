// Ragged correct for CDNA4 (gfx950): the locate launch (rs_locate_ragged.hip)
// that also FIXES what it names, in place -- slime_rs_plan_correct_batch over
// symbols, slime_rs_correct_objects_batch over stored chunk bytes, and their
// plan-set twins; max_wrong picks the one-shard rule or the pair rule behind it
// (PAIRS).  Every column the rule names is rewritten by correct_rule.hpp, so a
// following verify finds it clean; counts / first keep locate's shape and
// meaning and read "columns corrected in this shard", `unlocated` is what is
// left for erasure repair.  A named input whose coefficient column has no
// non-zero word (only a slime_rs_plan_matrix plan has one) cannot be solved:
// nothing is written and the column counts as unlocated.
//
// Fast path -- locate's, the same helpers (rs_locate_ragged_kernel.hpp):
// UnitWalk over the batch's unit list, load_tile, flag_tile, the filter, a
// static walk one step at a time, 1024 blocks.  Clean data is never written.
//
// Rare path -- the lane that holds a flagged column classifies it
// (classify_column / classify_pair_column, the pair form with its LDS strip of
// syndromes) and then, for a named column, takes the Fix of correct_rule.hpp,
// forms every new word from the column as it is stored -- an input's residue
// plus its delta, an output row recomputed plus its delta -- and only then
// stores them, with plain 4-byte stores: canonical residues for symbols,
// BE(sym ^ mapping[o]) for bytes.  Tail items do the same, a column a lane.
// The one-shard form has no strip: the one syndrome an input's fix needs is
// recomputed.  No per-row arrays, no scratch, no inline assembly.
//
// Why this does not race: a column belongs to exactly one lane of the launch
// -- the unit list and the tail items partition every object's columns, and the
// lanes a step clips past a tile's end re-read a vector of their own wave's
// step and drop it.  A fix reads and writes only its own column's words.  The
// walk goes one step at a time, so when the rare path runs the lane has no load
// of another step in flight, and the stores precede the next step's loads in
// program order.  `in` and `cmp` are therefore plain pointers -- not const, not
// __restrict__, possibly the same buffer -- so that no load of them is taken
// for invariant (the scalar-cache path of const __restrict__ loads).  The
// caller's side of the argument: the shards a plan touches, and the objects of
// a batch, do not overlap in memory.
//
// Forms as locate: k <= 16 over 4-byte aligned bases, four columns a lane
// (K = 1..16, R = 2 / 4, SET, BYTES, both rules); otherwise one column a lane.
// One kernel signature serves plans and sets (SET: coeff is the table, the
// index arrays are null, rows is max_rows).
#include <hip/hip_runtime.h>

#include "correct_rule.hpp"
#include "kernels.hpp"
#include "rs_locate_ragged_kernel.hpp"
#include "rs_ragged_launch.hpp"
#include "verify_step.hpp"

namespace slime {
namespace correct {

using apply::kBlock;
using apply::kWaves;
using apply::u32x16;
using locate::kNoSlot;
using locate::Slots;
using ragged::Desc;
using ragged::ObjRef;
using ragged::PlanRef;
using ragged::PlanRows;
using ragged::Tail;
using ragged::Unit;
using ragged::UnitWalk;
using verify::be;
using verify::Tally;

// SLIME_RLOCATE_PARAMS with writable, possibly aliasing data pointers.
#define SLIME_RCORRECT_PARAMS                                                                                     \
  uint8_t *in, uint8_t *cmp, const Desc *__restrict__ descs, const Unit *__restrict__ units,                     \
      const Tail *__restrict__ tails, const uint32_t *__restrict__ coeff, const uint32_t *__restrict__ in_idx,   \
      const uint32_t *__restrict__ out_idx, const uint32_t *__restrict__ mapping,                                \
      const unsigned long long *__restrict__ filter, unsigned long long *__restrict__ counts,                    \
      unsigned long long *__restrict__ first, uint32_t nunits, uint64_t ntails, uint32_t rows, uint32_t k
#define SLIME_RCORRECT_PASS \
  in, cmp, descs, units, tails, coeff, in_idx, out_idx, mapping, filter, counts, first, nunits, ntails, rows, k

extern __shared__ uint32_t correct_strip[];  // PAIRS: rows x kBlock syndromes, [i][threadIdx.x]

// Classifies column `col` of the object at ib / cb as column_slots does and rewrites the words the
// rule names.  Returns the slots to tally: column_slots' answer, or `unlocated` for a named column
// that cannot be solved.  rows: the object's own plan's; max_rows: the set's, for set_slot.
template <bool PAIRS, bool SET, bool BYTES>
__device__ __forceinline__ Slots correct_column(uint8_t* ib, uint8_t* cb, const uint32_t* __restrict__ coeff,
                                                const uint32_t* __restrict__ in_idx, uint64_t in_shard,
                                                const uint32_t* __restrict__ out_idx, uint64_t cmp_shard,
                                                uint32_t rows, uint32_t k, uint32_t m, uint64_t col,
                                                uint32_t max_rows, uint32_t* strip) {
  const Slots ps = locate::column_slots<PAIRS, SET, BYTES>(ib, cb, coeff, in_idx, in_shard, out_idx, cmp_shard, rows,
                                                           k, m, col, max_rows, strip);
  const uint32_t unlocated = k + (SET ? max_rows : rows);
  if (ps.a == kNoSlot || ps.a == unlocated) return ps;
  const uint32_t cs = apply::wide_coeff_stride(k);
  auto in_ptr = [&](uint32_t j) {
    return reinterpret_cast<uint32_t*>(ib + (uint64_t)in_idx[j] * in_shard + (col << 2));
  };
  auto out_ptr = [&](uint32_t i) {
    return reinterpret_cast<uint32_t*>(cb + (uint64_t)out_idx[i] * cmp_shard + (col << 2));
  };
  auto in_word = [&](uint32_t j) {
    const uint32_t v = *in_ptr(j);
    return BYTES ? be(v) ^ m : v;
  };
  auto computed = [&](uint32_t i) { return apply::wide_dot(coeff + (uint64_t)i * cs, k, in_word); };
  auto c = [&](uint32_t i, uint32_t j) { return coeff[(uint64_t)i * cs + j]; };
  auto s = [&](uint32_t i) {
    if constexpr (PAIRS) {
      return strip[i * kBlock + threadIdx.x];  // classify_pair_column left it there
    } else {
      const uint32_t w = *out_ptr(i);
      return locate::sub(canon(BYTES ? be(w) ^ m : w), computed(i));
    }
  };
  const Fix f = ps.b == kNoSlot ? single_fix(s, c, k, rows, ps.a) : pair_fix(s, c, k, rows, ps.a, ps.b);
  if (!f.solved) return Slots{unlocated, kNoSlot};
  // Every new word from the column as stored, then the stores.
  auto value = [&](uint32_t slot, uint32_t d) {
    return locate::add(slot < k ? canon(in_word(slot)) : computed(slot - k), d);
  };
  auto put = [&](uint32_t slot, uint32_t v) { *(slot < k ? in_ptr(slot) : out_ptr(slot - k)) = BYTES ? be(v ^ m) : v; };
  const uint32_t va = value(ps.a, f.da);
  if (ps.b != kNoSlot) put(ps.b, value(ps.b, f.db));
  put(ps.a, va);
  return ps;
}

// locate_tails with the fix: one {object, column} per lane.
template <bool PAIRS, bool SET, bool BYTES>
__device__ __forceinline__ void correct_tails(SLIME_RCORRECT_PARAMS, uint32_t* strip) {
  const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t nthr = (uint64_t)gridDim.x * kBlock;
  const uint32_t nslots = k + rows + 1;
  for (uint64_t t = tid; t < ntails; t += nthr) {
    const Tail it = tails[t];
    if (locate::filtered_out(filter, it.obj, rows)) continue;
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
    const Slots ps = correct_column<PAIRS, SET, BYTES>(in + (d->src_off << 2), cmp + (d->dst_off << 2), pl.coeff, iidx,
                                                       d->src_shard << 2, pl.oidx, d->dst_shard << 2, pl.rows, k, m,
                                                       it.col, rows, strip);
    if (ps.a != kNoSlot) {
      atomicAdd(counts + (uint64_t)it.obj * nslots + ps.a, 1ull);
      atomicMin(first + (uint64_t)it.obj * nslots + ps.a, (unsigned long long)it.col);
    }
    if constexpr (PAIRS) {
      if (ps.b != kNoSlot) {
        atomicAdd(counts + (uint64_t)it.obj * nslots + ps.b, 1ull);
        atomicMin(first + (uint64_t)it.obj * nslots + ps.b, (unsigned long long)it.col);
      }
    }
  }
}

// locate_vectors with the fix on its rare path: four columns a lane, k = K <= 16.
template <bool PAIRS, int K, int W, int R, int UB, int C, bool SET, bool BYTES>
__device__ __forceinline__ void correct_vectors(SLIME_RCORRECT_PARAMS, uint32_t* strip) {
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
  uint8_t* ib = in;
  uint8_t* cb = cmp;
  uint64_t ishard = 0, cshard = 0;
  uint32_t m = 0;
  PlanRows pl{coeff, SET ? coeff : out_idx, SET ? 1 : rows};
  const uint32_t* iidx = SET ? coeff : in_idx;
  bool skip = false;
  while (w.live) {
    if (w.fresh) {  // the first tile since the object changed
      skip = locate::filtered_out(filter, w.obj, rows);
      if (!skip) {
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
        const uint32_t bits = locate::flag_tile<K, W, R, BYTES, uint32_t>(x, s, cb, pl.coeff, pl.oidx, cshard, pl.rows,
                                                                          m, tb, tend, lane);
        if (__ballot(bits != 0)) {
          // Rare path: word q & 3 of unit q >> 2, every lane that flagged it, in column order.
          for (uint32_t q = 0; q < 4u * W; ++q) {
            const bool hit = (bits >> q) & 1u;
            if (!__ballot(hit)) continue;
            const uint64_t col = ((uint64_t)(tb + 64 * (q >> 2) + lane) << 2) + (q & 3u);
            Slots ps{kNoSlot, kNoSlot};
            if (hit)
              ps = correct_column<PAIRS, SET, BYTES>(ib, cb, pl.coeff, iidx, ishard, pl.oidx, cshard, pl.rows, k, m,
                                                     col, rows, strip);
            locate::tally_slots(t, ps.a, col);
            if constexpr (PAIRS) locate::tally_slots(t, ps.b, col);
          }
        }
      }
    }
    w.advance();
  }
  t.flush();
  correct_tails<PAIRS, SET, BYTES>(SLIME_RCORRECT_PASS, strip);
}

// locate_columns with the fix: one column a lane, generic k, any alignment.
template <bool PAIRS, bool SET, bool BYTES>
__device__ __forceinline__ void correct_columns(SLIME_RCORRECT_PARAMS, uint32_t tile_cols, uint32_t unit_tiles,
                                                uint32_t* strip) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * kWaves;
  const uint32_t nslots = k + rows + 1, cs = apply::wide_coeff_stride(k);
  Tally t(lane);
  for (uint64_t e = wave; e < nunits; e += nwaves) {
    const Unit u = units[e];
    if (locate::filtered_out(filter, u.obj, rows)) continue;
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
    uint8_t* const ib = in + (d.src_off << 2);
    uint8_t* const cb = cmp + (d.dst_off << 2);
    const uint64_t ishard = d.src_shard << 2, cshard = d.dst_shard << 2;
    for (uint64_t bw = c.b0; bw < c.b1; bw += 64) {
      // bw is always inside the object; lanes past the last column re-read column bw -- their own
      // wave's, before its fix -- and never count.
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
          ps = correct_column<PAIRS, SET, BYTES>(ib, cb, pl.coeff, iidx, ishard, pl.oidx, cshard, pl.rows, k, m, col,
                                                 rows, strip);
        locate::tally_slots(t, ps.a, col);
        if constexpr (PAIRS) locate::tally_slots(t, ps.b, col);
      }
    }
  }
  t.flush();
  correct_tails<PAIRS, SET, BYTES>(SLIME_RCORRECT_PASS, strip);
}

template <bool PAIRS, int K, int W, int R, int UB, int C, bool SET, bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_correct_ragged_kernel(SLIME_RCORRECT_PARAMS) {
  correct_vectors<PAIRS, K, W, R, UB, C, SET, BYTES>(SLIME_RCORRECT_PASS, PAIRS ? correct_strip : nullptr);
}

template <bool PAIRS, bool SET, bool BYTES>
__global__ __launch_bounds__(kBlock) void rs_correct_ragged_column_kernel(SLIME_RCORRECT_PARAMS, uint32_t tile_cols,
                                                                          uint32_t unit_tiles) {
  correct_columns<PAIRS, SET, BYTES>(SLIME_RCORRECT_PASS, tile_cols, unit_tiles, PAIRS ? correct_strip : nullptr);
}

}  // namespace correct

namespace {

using apply::kBlock;

// (v).p.rows is the plan's rows or the set's max_rows; a set passes its table and no index arrays.
#define SLIME_RCORRECT_ARGS(v)                                                                                  \
  (uint8_t*)(v).in, (uint8_t*)(v).cmp, (v).w.desc, (v).w.units, (v).w.tails, SET ? (v).p.table : (v).p.coeff,   \
      SET ? nullptr : (v).p.in_idx, SET ? nullptr : (v).p.out_idx, (v).mapping,                                 \
      (const unsigned long long*)(v).filter, (unsigned long long*)(v).counts, (unsigned long long*)(v).first,   \
      (v).w.nunits, (v).w.ntails, (v).p.rows, (v).w.k

constexpr uint64_t kCorrectBlocks = 1024;  // locate's: four blocks a CU

// The dynamic LDS of a block: the pair rule's strip, one word per row and thread (k + rows <= 63:
// at most 62 rows, 62 KiB, under the 64 KiB a block may always ask for).
template <bool PAIRS>
uint32_t strip_bytes(const RaggedCorrectLaunch& v) {
  return PAIRS ? v.p.rows * kBlock * (uint32_t)sizeof(uint32_t) : 0;
}

template <int K, int R, bool PAIRS, bool SET, bool BYTES>
hipError_t launch_vectors(const RaggedCorrectLaunch& v, hipStream_t s) {
  constexpr int UB = ragged::unroll_for_k(K), C = ragged::unit_tiles_for_k(K), W = verify_step::width(K, R);
  const dim3 grid((uint32_t)ragged::ragged_blocks(kCorrectBlocks, v.w.nunits, v.w.ntails));
  hipLaunchKernelGGL((correct::rs_correct_ragged_kernel<PAIRS, K, W, R, UB, C, SET, BYTES>), grid, dim3(kBlock),
                     strip_bytes<PAIRS>(v), s, SLIME_RCORRECT_ARGS(v));
  return hipGetLastError();
}

// R -- the stored rows a step carries -- from the plan's rows or the set's max_rows; always 4
// with PAIRS, whose launches have rows >= 4.
template <int K, bool PAIRS, bool SET>
hipError_t launch_rows(const RaggedCorrectLaunch& v, hipStream_t s) {
  const bool bytes = v.mapping != nullptr;
  if constexpr (!PAIRS)
    if (verify_step::stored_rows(v.p.rows) == 2)
      return bytes ? launch_vectors<K, 2, false, SET, true>(v, s) : launch_vectors<K, 2, false, SET, false>(v, s);
  return bytes ? launch_vectors<K, 4, PAIRS, SET, true>(v, s) : launch_vectors<K, 4, PAIRS, SET, false>(v, s);
}

template <bool PAIRS, bool SET, bool BYTES>
hipError_t launch_columns(const RaggedCorrectLaunch& v, hipStream_t s) {
  const dim3 grid((uint32_t)ragged::ragged_blocks(kCorrectBlocks, v.w.nunits, v.w.ntails));
  const uint32_t tile_cols = 256u * (uint32_t)v.w.U, unit_tiles = (uint32_t)v.w.C;
  hipLaunchKernelGGL((correct::rs_correct_ragged_column_kernel<PAIRS, SET, BYTES>), grid, dim3(kBlock),
                     strip_bytes<PAIRS>(v), s, SLIME_RCORRECT_ARGS(v), tile_cols, unit_tiles);
  return hipGetLastError();
}

#undef SLIME_RCORRECT_ARGS

template <bool PAIRS, bool SET>
hipError_t launch_form(const RaggedCorrectLaunch& v, bool vec, hipStream_t s) {
  if (!vec) return v.mapping ? launch_columns<PAIRS, SET, true>(v, s) : launch_columns<PAIRS, SET, false>(v, s);
  return ragged::with_k(v.w.k, [&](auto kc) { return launch_rows<decltype(kc)::value, PAIRS, SET>(v, s); });
}

}  // namespace

hipError_t launch_correct_ragged(const RaggedCorrectLaunch& v, hipStream_t s) {
  (void)hipGetLastError();  // report only this launch's error, not one left on the thread
  if (v.w.nobj == 0) return hipSuccess;
  if (v.p.rows < (v.pairs ? locate::kPairRows : 2u) || v.w.k + v.p.rows > locate::kMaxSlots)
    return hipErrorInvalidValue;
  if (hipError_t e = launch_verify_init(v.counts, v.first, v.w.nobj * (v.w.k + v.p.rows + 1), s)) return e;
  if (v.w.nunits == 0 && v.w.ntails == 0) return hipSuccess;  // an empty batch: nothing but the initialisation
  const bool vec = v.w.k <= 16 && v.w.vec_ok;
  // The vector kernels are instantiated with the geometry of their K: the tables must be cut by it.
  if (vec && (v.w.U != ragged::unroll_for_k((int)v.w.k) || v.w.C != ragged::unit_tiles_for_k((int)v.w.k)))
    return hipErrorInvalidValue;
  if (v.pairs) return v.p.table ? launch_form<true, true>(v, vec, s) : launch_form<true, false>(v, vec, s);
  return v.p.table ? launch_form<false, true>(v, vec, s) : launch_form<false, false>(v, vec, s);
}

}  // namespace slime
