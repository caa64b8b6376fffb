// A wave's walk over the unit list of a ragged batch (ragged_plan.hpp), and
// the per-object loads that go with it: the object's descriptor and, in a
// planned batch, the record of its plan in a plan set's table
// (planset_table.hpp); for the generic-k column kernels, which walk the list
// without UnitWalk, a unit's column range (unit_columns).  Shared by every
// ragged launch: apply (rs_ragged.hip), verify (rs_verify_ragged.hip), locate
// (rs_locate_ragged.hip) and the byte forms (rs_bytes_ragged.hip,
// rs_bytes_ragged_encode.hip); rs_ragged.hip's header comment describes the
// walk.
#pragma once
#include <hip/hip_runtime.h>

#include "planset_table.hpp"
#include "ragged_plan.hpp"
#include "rs_apply_kernel.hpp"

namespace slime {
namespace ragged {

using apply::kBlock;
using apply::kTicketStride;
using apply::kWaves;
using apply::u32x16;

// A descriptor's live fields in SGPRs.
struct ObjRef {
  uint64_t src_off, src_shard, dst_off, dst_shard;
  uint32_t nvec, ntiles;
};
__device__ __forceinline__ ObjRef load_desc(const Desc* __restrict__ descs, uint32_t obj) {
  const u32x16 v = *reinterpret_cast<const u32x16*>(descs + obj);  // one 64-byte entry
  ObjRef r;
  r.src_off = v[0] | ((uint64_t)v[1] << 32);
  r.src_shard = v[2] | ((uint64_t)v[3] << 32);
  r.dst_off = v[4] | ((uint64_t)v[5] << 32);
  r.dst_shard = v[6] | ((uint64_t)v[7] << 32);
  r.nvec = v[8];
  r.ntiles = v[9];
  return r;
}

// The columns [b0, b1) of unit u in an object of `ntiles` tiles, as the
// generic-k column kernels read them: tile_cols columns a tile, up to
// unit_tiles tiles from u.tile on, cut at vector `nvec` (the object's whole
// vectors; byte encode passes its interior bound).  The unit goes by value:
// by reference the apply's single-plan column kernel compiles to other bytes.
struct ColRange {
  uint64_t b0, b1;
};
__device__ __forceinline__ ColRange unit_columns(uint32_t ntiles, const Unit u, uint32_t tile_cols,
                                                 uint32_t unit_tiles, uint32_t nvec) {
  const uint32_t t1 = ntiles - u.tile < unit_tiles ? ntiles : u.tile + unit_tiles;
  const uint64_t b0 = (uint64_t)u.tile * tile_cols, bmax = (uint64_t)nvec << 2;
  const uint64_t b1 = (uint64_t)t1 * tile_cols < bmax ? (uint64_t)t1 * tile_cols : bmax;
  return ColRange{b0, b1};
}

// A wave's walk over the unit list (device state, wave-uniform), with
// TicketWalk's interface: obj, tile(), advance(), live, finish() -- and d,
// the current object's descriptor, with `fresh` set while the current tile is
// the first since d changed.
template <int C, int NC, bool DYN>
struct UnitWalk {
  uint32_t* ticket;
  const Unit* __restrict__ list;
  const Desc* __restrict__ descs;
  uint32_t n, ngrp, lane;          // list entries; groups of four entries, ceil(n / 4)
  uint32_t p = 0, dry = 0, pend = 0;  // DYN: partition, partitions found dry, pending atomic
  uint32_t e = 0, step = 0;           // static: the entry loaded ahead, the wave count
  uint32_t a_obj = 0, a_tile = 0;     // the next unit's entry (loaded a unit ahead)
  bool a_ok = false;
  ObjRef d{};
  uint32_t d_obj = ~0u;
  bool fresh = false;
  uint32_t obj = 0, tb = 0, cnt = 0, i = 0;  // current unit
  bool live = true;

  // first / step_: the wave's index and the launch's wave count (static walk).
  __device__ __forceinline__ UnitWalk(uint32_t* t, const Unit* __restrict__ list_, const Desc* __restrict__ descs_,
                                      uint32_t n_, uint32_t lane_, uint32_t first, uint32_t step_)
      : ticket(t), list(list_), descs(descs_), n(n_), ngrp(list_groups(n_)), lane(lane_) {
    uint32_t en = 0;
    if constexpr (DYN) {
      p = hw_xcc() % NC;
      a_ok = skip_empty();
      if (a_ok) {
        request();
        a_ok = draw(en);
      }
    } else {
      step = step_;
      e = first;
      a_ok = e < n;
      en = e;
    }
    if (a_ok) load_ahead(en);
    next_unit();
  }
  __device__ __forceinline__ static uint32_t hw_xcc() { return apply::hw_xcc_id(); }
  // TicketWalk::skip_empty: partition p holds units iff p < ngrp.
  __device__ __forceinline__ bool skip_empty() {
    if (p < ngrp) return true;
    dry += NC - p;
    p = 0;
    return ngrp != 0 && dry < NC;  // false: every partition is dry
  }
  __device__ __forceinline__ void request() {
    pend = 0;
    if (lane == 0) pend = atomicAdd(ticket + p * kTicketStride, 1u);
  }
  // The list index of the pending ticket (or of a later one: dry partitions
  // and the last group's missing entries are passed over), and the request of
  // the ticket after it.  false: every partition is dry, no draw is pending.
  __device__ __forceinline__ bool draw(uint32_t& en) {
    for (;;) {
      const uint32_t l = __builtin_amdgcn_readlane(pend, 0);  // lane 0 drew it, whatever the exec mask
      if (l >= partition_tickets(ngrp, p, NC)) {
        if (++dry >= NC) return false;
        p = p + 1 == NC ? 0 : p + 1;
        if (!skip_empty()) return false;
        request();
        continue;
      }
      request();
      en = ticket_entry(l, p, NC);
      if (en < n) return true;
    }
  }
  __device__ __forceinline__ void load_ahead(uint32_t en) {
    const uint2 v = *reinterpret_cast<const uint2*>(list + en);  // one 8-byte scalar load
    a_obj = v.x;
    a_tile = v.y;
  }
  // Enter the unit loaded ahead, and fetch the entry of the one after it.
  __device__ __forceinline__ void next_unit() {
    if (!a_ok) {
      live = false;
      return;
    }
    obj = a_obj;
    tb = a_tile;
    i = 0;
    uint32_t en = 0;
    if constexpr (DYN) {
      a_ok = draw(en);
    } else {
      a_ok = n - e > step;  // e + step < n, no wrap
      e += step;
      en = e;
    }
    if (a_ok) load_ahead(en);
    if (obj != d_obj) {
      d = load_desc(descs, obj);
      d_obj = obj;
      fresh = true;
    }
    cnt = d.ntiles - tb < (uint32_t)C ? d.ntiles - tb : (uint32_t)C;  // the host lists tb < ntiles only
  }
  __device__ __forceinline__ uint32_t tile() const { return tb + i; }
  __device__ __forceinline__ void advance() {
    fresh = false;
    if (++i >= cnt) next_unit();
  }
  // TicketWalk::finish: once per wave after the walk ended; the launch's last
  // wave out returns the counter set to zero.
  __device__ __forceinline__ void finish() {
    if constexpr (DYN) {
      if (lane == 0) {
        uint32_t* const done = ticket + NC * kTicketStride;
        if (atomicAdd(done, 1u) == gridDim.x * gridDim.y * (blockDim.x >> 6) - 1) {
#pragma unroll
          for (int q = 0; q < NC; ++q) atomicExch(ticket + q * kTicketStride, 0u);
          atomicExch(done, 0u);
        }
      }
    }
  }
};

// A plan record's live fields in SGPRs.
struct PlanRef {
  uint32_t rows, in_off, out_off, coeff_off;
};
// The record of object obj's plan: the index from the descriptor's line (which
// the walk has just loaded; ObjRef and load_desc stay as the single-plan
// kernels compile them), then the record, two dependent scalar loads.
__device__ __forceinline__ PlanRef load_plan(const uint32_t* __restrict__ tab, const Desc* __restrict__ descs,
                                             uint32_t obj) {
  const uint32_t plan = descs[obj].reserved[0];
  const apply::u32x4 v = *reinterpret_cast<const apply::u32x4*>(tab + (uint64_t)plan * planset::kRecordWords);
  return PlanRef{v[0], v[1], v[2], v[3]};
}
// The same record read by ONE LANE through its item's descriptor (the tail
// items: neighbouring lanes hold different objects).
__device__ __forceinline__ PlanRef read_plan(const uint32_t* __restrict__ tab, const Desc* d) {
  const uint32_t* const rec = tab + (uint64_t)d->reserved[0] * planset::kRecordWords;
  return PlanRef{rec[0], rec[1], rec[2], rec[3]};
}

// A plan's rows as a launch reads them (verify: one row block of the plan).
struct PlanRows {
  const uint32_t* coeff;
  const uint32_t* oidx;
  uint32_t rows;
};
// The rows of a plan that fall into a verify launch's row block [r0, r0 + 64).
__device__ __forceinline__ uint32_t block_rows(uint32_t rows, uint32_t r0) {
  return rows > r0 ? (rows - r0 < 64u ? rows - r0 : 64u) : 0u;
}
// The plan with record p of the set's table `tab`, whole (byte decode); its
// input indices are at tab + p.in_off.  Verify reads one row block of it
// (rs_verify_ragged_kernel.hpp).
__device__ __forceinline__ PlanRows whole_plan(const uint32_t* tab, const PlanRef& p) {
  return PlanRows{tab + p.coeff_off, tab + p.out_off, p.rows};
}

}  // namespace ragged
}  // namespace slime
