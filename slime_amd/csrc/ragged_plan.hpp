// Host work tables of a ragged batch (slime_rs_batch_create): one launch over
// objects of different lengths at arbitrary offsets.  Pure host code, no HIP:
// tests/cpp/ragged_plan_test.cpp builds it with plain g++.
//
// For a tile geometry (U, C) -- a tile is 64 U 16-byte vectors (256 U columns)
// of every shard, a unit up to C consecutive tiles of ONE object -- the spans
// become three tables the kernels of rs_ragged.hip read from device memory:
//   descriptors  one 64-byte entry per object (its offsets, strides, vector
//                and tile counts), 64 bytes apart, so a wave takes an entry
//                with one 16-dword scalar load;
//   units        one 8-byte entry {object, first tile} per unit; objects of
//                fewer than 4 columns have none.  The objects are cut into
//                about `segments` contiguous segments of equal length over
//                the batch (a short object is one segment), and the list
//                goes round the segments, four consecutive units (one ticket
//                group, 4 C tiles) of each in turn: the groups running at
//                any moment spread over the batch as the uniform launch's
//                do (TicketWalk and its `spread`, rs_apply_kernel.hpp).
//                Listed object after object, the same kernel ran 8/12 over
//                128 x 256 MiB objects at 9.30 ms against 8.22 ms for the
//                uniform launch;
//   tails        one 8-byte entry {object, column} per column past an
//                object's last whole vector (L % 4 of them, all L columns of
//                an object shorter than a vector).
// A ticket of the dynamic walk (or a wave's stride of the static one) indexes
// the unit list directly: no search over a prefix array in front of a unit.
// Size: 8 bytes per unit of up to 256 U C columns of k + rows shards -- a full
// unit moves 60 KiB at 3/5 (U = 4, C = 3: 12 KiB a shard), 72 KiB at 8/12 and
// 120 KiB at 16/20 (6 KiB a shard) -- plus 64 bytes per object: 10^5 objects
// holding 64 GiB of shards are a unit list under 10 MB beside 6.4 MB of
// descriptors.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace slime {
namespace ragged {

// One object of a batch (the layout of slime_rs_span_t, include/slime_rs.h):
// offsets and strides in uint32 elements from the launch's src / dst.
struct Span {
  uint64_t src_off, src_shard_stride, dst_off, dst_shard_stride, L;
};

// Shards of a ragged batch stay under 4 GiB: the kernels keep 32-bit byte
// offsets inside a shard (the uniform API remains for larger ones).
constexpr uint64_t kMaxL = 1ull << 30;

// Tile geometry by the number of inputs k, the dynamic-schedule apply
// launch's (rs_apply.hip, launch_queue): 16-byte vectors per lane per tile
// and tiles per unit.  Codes wider than 16 inputs run one column per lane
// over the tiles of k = 16.
constexpr int unroll_for_k(int k) { return k <= 4 ? 4 : k <= 12 ? 3 : 1; }
constexpr int unit_tiles_for_k(int k) { return k <= 4 ? 3 : k <= 12 ? 2 : 6; }
// Segments the unit list goes round (build()): the dynamic-schedule apply
// launch's `spread` rule (queue_spread, kernels.hpp) -- about 64 windows over
// the batch, 256 for the six-stream code 4/6 -- keyed by k alone, since a
// batch serves every plan with k inputs.
constexpr uint32_t segments_for_k(int k) { return k == 4 ? 256u : 64u; }
struct Geometry {
  int U, C;
  uint32_t segments;
};
constexpr Geometry geometry_for_k(int k) { return Geometry{unroll_for_k(k), unit_tiles_for_k(k), segments_for_k(k)}; }

struct alignas(64) Desc {
  uint64_t src_off, src_shard, dst_off, dst_shard;  // uint32 elements
  uint32_t nvec;                                    // whole 16-byte vectors per shard, L / 4
  uint32_t ntiles;                                  // ceil(nvec / 64 U)
  uint32_t ncols;                                   // L
  uint32_t reserved[5];                             // [0]: the object's plan index in a planned batch, else zero
};
static_assert(sizeof(Desc) == 64 && alignof(Desc) == 64, "one s_load_dwordx16 per descriptor");

struct Unit {
  uint32_t obj, tile;  // tiles [tile, min(tile + C, ntiles of obj))
};
struct Tail {
  uint32_t obj, col;
};
static_assert(sizeof(Unit) == 8 && sizeof(Tail) == 8, "8-byte list entries");

// The dynamic walk's dealing of the unit list over NC ticket counters
// (UnitWalk, rs_ragged_walk.hpp; TicketWalk's, rs_apply_kernel.hpp): the list is
// cut into groups of four consecutive entries, group g belongs to partition
// g % NC, and ticket l of partition p is entry l % 4 of the partition's
// (l / 4)-th group.  A partition hands out 4 tickets per group it owns; the
// last group's entries past the list's end are drawn and passed over.
#ifdef __HIPCC__
#define SLIME_RAGGED_HD __host__ __device__
#else
#define SLIME_RAGGED_HD
#endif
SLIME_RAGGED_HD inline uint32_t list_groups(uint32_t n) { return n / 4 + (n % 4 ? 1 : 0); }
SLIME_RAGGED_HD inline uint32_t partition_tickets(uint32_t ngrp, uint32_t p, uint32_t nc) {
  return 4 * ((ngrp + nc - 1 - p) / nc);
}
// Entry of ticket l < partition_tickets(ngrp, p, nc): below 4 ngrp <= 2^32, so no wrap.
SLIME_RAGGED_HD inline uint32_t ticket_entry(uint32_t l, uint32_t p, uint32_t nc) {
  return ((l >> 2) * nc + p) * 4 + (l & 3);
}

// A planned batch (slime_rs_batch_create_planned) names one plan of a plan set
// (planset_table.hpp) per object: plan_of[o] < nplans goes into the
// descriptor's first reserved word; kNoPlan marks an intact object, which
// gets no units and no tails, exactly like L == 0.
constexpr uint32_t kNoPlan = 0xFFFFFFFFu;

struct Counts {
  uint64_t nobj = 0, columns = 0, tiles = 0, units = 0, tails = 0;
};

inline uint64_t tiles_of(uint64_t L, int U) { return ((L >> 2) + 64ull * U - 1) / (64ull * U); }
inline uint64_t units_of(uint64_t L, Geometry g) { return (tiles_of(L, g.U) + g.C - 1) / g.C; }
inline uint64_t tails_of(uint64_t L) { return L & 3; }

// Validates the spans and counts what build() would make, allocating nothing.
// false: *why names the refusal.
// plan_of (optional): nobj plan indices below nplans, or kNoPlan.
inline bool count(const Span* spans, uint64_t nobj, Geometry g, Counts* out, std::string* why,
                  const uint32_t* plan_of = nullptr, uint32_t nplans = 0) {
  Counts c;
  c.nobj = nobj;
  if (nobj > 0xFFFFFFFFull) {
    *why = "nobj exceeds 2^32-1";
    return false;
  }
  for (uint64_t o = 0; o < nobj; ++o) {
    const uint64_t L = spans[o].L;
    if (L >= kMaxL) {
      *why = "span " + std::to_string(o) + ": L = " + std::to_string(L) +
             " is 2^30 or more (a ragged batch keeps shards under 4 GiB; use slime_rs_plan_execute)";
      return false;
    }
    if (plan_of) {
      if (plan_of[o] == kNoPlan) continue;
      if (plan_of[o] >= nplans) {
        *why = "span " + std::to_string(o) + ": plan index " + std::to_string(plan_of[o]) + " of a set of " +
               std::to_string(nplans);
        return false;
      }
    }
    c.columns += L;
    c.tiles += tiles_of(L, g.U);
    c.units += units_of(L, g);
    c.tails += tails_of(L);
  }
  if (c.units >= (1ull << 32)) {
    *why = std::to_string(c.units) + " units: a ragged batch holds fewer than 2^32 (split the batch)";
    return false;
  }
  *out = c;
  return true;
}

struct Tables {
  Geometry g{1, 1};
  Counts counts;
  std::vector<Desc> desc;
  std::vector<Unit> units;
  std::vector<Tail> tails;
};

inline bool build(const Span* spans, uint64_t nobj, Geometry g, Tables* t, std::string* why,
                  const uint32_t* plan_of = nullptr, uint32_t nplans = 0) {
  if (!count(spans, nobj, g, &t->counts, why, plan_of, nplans)) return false;
  // The columns of object o that the launch works on: none of an intact object.
  auto len = [&](uint64_t o) { return plan_of && plan_of[o] == kNoPlan ? 0ull : spans[o].L; };
  t->g = g;
  t->desc.assign(nobj, Desc{});
  t->units.clear();
  t->tails.clear();
  t->units.reserve(t->counts.units);
  t->tails.reserve(t->counts.tails);
  // Segment length: whole ticket groups (4 units, 4 C tiles), the batch's groups over `segments`.
  uint64_t groups = 0;
  for (uint64_t o = 0; o < nobj; ++o) groups += (units_of(len(o), g) + 3) / 4;
  const uint64_t nseg = g.segments ? g.segments : 1;
  const uint64_t seg_groups = groups > nseg ? (groups + nseg - 1) / nseg : 1;
  const uint64_t seg_tiles = seg_groups * 4 * (uint64_t)g.C;
  struct Seg {
    uint32_t obj, next, end;  // tiles [next, end) left to list
  };
  std::vector<Seg> live;
  for (uint64_t o = 0; o < nobj; ++o) {
    const Span& s = spans[o];
    const uint64_t L = len(o);
    Desc& d = t->desc[o];
    d.src_off = s.src_off;
    d.src_shard = s.src_shard_stride;
    d.dst_off = s.dst_off;
    d.dst_shard = s.dst_shard_stride;
    d.nvec = (uint32_t)(L >> 2);
    d.ntiles = (uint32_t)tiles_of(L, g.U);
    d.ncols = (uint32_t)L;
    d.reserved[0] = plan_of ? plan_of[o] : 0u;
    for (uint64_t t0 = 0; t0 < d.ntiles; t0 += seg_tiles)
      live.push_back(Seg{(uint32_t)o, (uint32_t)t0, (uint32_t)(t0 + seg_tiles < d.ntiles ? t0 + seg_tiles : d.ntiles)});
    for (uint64_t b = (uint64_t)d.nvec << 2; b < L; ++b) t->tails.push_back(Tail{(uint32_t)o, (uint32_t)b});
  }
  // Round after round over the segments that have units left, four units each.
  while (!live.empty()) {
    size_t keep = 0;
    for (Seg sg : live) {
      for (int q = 0; q < 4 && sg.next < sg.end; ++q, sg.next += (uint32_t)g.C) t->units.push_back(Unit{sg.obj, sg.next});
      if (sg.next < sg.end) live[keep++] = sg;
    }
    live.resize(keep);
  }
  return true;
}

}  // namespace ragged
}  // namespace slime
