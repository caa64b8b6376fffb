// CPU test of the ragged batch's host work tables (slime_amd/csrc/ragged_plan.hpp),
// the three tables slime_rs_batch_create uploads and the kernels of
// rs_ragged.hip walk.  For every tile geometry (U, C) the library uses, over
// hand-made and random span lists:
//
//   - every (object, tile) pair is in exactly one unit, no unit crosses an
//     object, a unit has at most C tiles and starts on a multiple of C; the
//     list goes round the batch's segments four units at a time (two small
//     examples spelled out);
//   - objects of fewer than 4 columns (empty ones included) have no unit, and
//     every column past an object's last whole vector is listed exactly once
//     as a tail item, nothing else is;
//   - descriptors are 64 bytes apart and carry the span and its counts;
//   - the dynamic walk's dealing (partition_tickets / ticket_entry) hands out
//     every list entry exactly once over the eight ticket counters;
//   - creation refuses L = 2^30, and a span list whose unit count reaches 2^32
//     (counted, never allocated).
// Usage: ragged_plan_test   (exit 0 = pass)
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "ragged_plan.hpp"

using namespace slime::ragged;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

namespace {

// The geometries geometry_for_k yields over every k a plan allows.
std::vector<Geometry> geometries() {
  std::set<std::tuple<int, int, uint32_t>> seen;
  std::vector<Geometry> out;
  for (int k = 1; k <= 128; ++k) {
    const Geometry g = geometry_for_k(k);
    if (seen.insert({g.U, g.C, g.segments}).second) out.push_back(g);
  }
  return out;
}

void check_tables(const std::vector<Span>& spans, Geometry g) {
  Tables t;
  std::string why;
  CHECK(build(spans.data(), spans.size(), g, &t, &why));
  const uint64_t T = 256ull * g.U;  // columns per tile
  CHECK(t.desc.size() == spans.size());
  CHECK(t.counts.nobj == spans.size());
  CHECK(t.counts.units == t.units.size() && t.counts.tails == t.tails.size());
  uint64_t columns = 0, tiles = 0;
  for (size_t o = 0; o < spans.size(); ++o) {
    const Desc& d = t.desc[o];
    CHECK((const char*)&t.desc[o] - (const char*)&t.desc[0] == (std::ptrdiff_t)(64 * o));
    CHECK(d.src_off == spans[o].src_off && d.src_shard == spans[o].src_shard_stride);
    CHECK(d.dst_off == spans[o].dst_off && d.dst_shard == spans[o].dst_shard_stride);
    CHECK(d.ncols == spans[o].L && d.nvec == spans[o].L / 4);
    CHECK(d.ntiles == (spans[o].L / 4 * 4 + T - 1) / T);
    for (uint32_t r : d.reserved) CHECK(r == 0);
    columns += spans[o].L;
    tiles += d.ntiles;
  }
  CHECK(t.counts.columns == columns && t.counts.tiles == tiles);
  // Units: every (object, tile) once; at most C tiles, from a multiple of C; inside one object.
  std::map<std::pair<uint32_t, uint32_t>, int> covered;
  for (size_t u = 0; u < t.units.size(); ++u) {
    const Unit& un = t.units[u];
    CHECK(un.obj < spans.size());
    const Desc& d = t.desc[un.obj];
    CHECK(d.nvec >= 1);  // an object of fewer than 4 columns has no unit
    CHECK(un.tile < d.ntiles);
    const uint32_t end = d.ntiles - un.tile < (uint32_t)g.C ? d.ntiles : un.tile + g.C;
    CHECK(end > un.tile && end - un.tile <= (uint32_t)g.C);
    for (uint32_t tile = un.tile; tile < end; ++tile) ++covered[{un.obj, tile}];
    CHECK(un.tile % (uint32_t)g.C == 0);
  }
  CHECK(covered.size() == tiles);
  for (const auto& kv : covered) CHECK(kv.second == 1);
  for (size_t o = 0; o < spans.size(); ++o)
    for (uint32_t tile = 0; tile < t.desc[o].ntiles; ++tile) CHECK(covered.count({(uint32_t)o, tile}) == 1);
  // Tails: exactly the columns [4 nvec, L) of every object, once each.
  std::set<std::pair<uint32_t, uint32_t>> tails;
  for (const Tail& tl : t.tails) {
    CHECK(tl.obj < spans.size());
    CHECK(tl.col >= t.desc[tl.obj].nvec * 4 && tl.col < spans[tl.obj].L);
    CHECK(tails.insert({tl.obj, tl.col}).second);
  }
  uint64_t want_tails = 0;
  for (const Span& s : spans) want_tails += s.L % 4;
  CHECK(tails.size() == want_tails);
  // Dealing: the tickets of the 8 partitions name every list entry once.
  const uint32_t n = (uint32_t)t.units.size(), ngrp = list_groups(n), NC = 8;
  std::vector<int> drawn(n, 0);
  uint64_t beyond = 0;
  for (uint32_t p = 0; p < NC; ++p)
    for (uint32_t l = 0; l < partition_tickets(ngrp, p, NC); ++l) {
      const uint32_t e = ticket_entry(l, p, NC);
      CHECK(e < 4 * (uint64_t)ngrp);
      if (e < n)
        ++drawn[e];
      else
        ++beyond;
    }
  for (int c : drawn) CHECK(c == 1);
  CHECK(beyond == 4 * (uint64_t)ngrp - n);
}

Span span_of(uint64_t L, uint64_t off) { return Span{off, L + 3, off + 7, L + 5, L}; }

void TestHandMade() {
  for (const Geometry g : geometries()) {
    const uint64_t T = 256ull * g.U, C = g.C;
    const uint64_t lens[] = {0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 257, T - 1, T, T + 1, T + 4, C * T - 1, C * T,
                             C * T + 1, C * T + 4, 4 * C * T + 5, 0, 3};
    std::vector<Span> spans;
    uint64_t off = 11;
    for (uint64_t L : lens) {
      spans.push_back(span_of(L, off));
      off += 20 * (L + 5);
    }
    check_tables(spans, g);
    // Each alone, and none at all.
    for (const Span& s : spans) check_tables({s}, g);
    check_tables({}, g);
    // Objects of fewer than 4 columns only: no unit, every column a tail.
    Tables t;
    std::string why;
    const std::vector<Span> tiny = {span_of(0, 0), span_of(1, 10), span_of(2, 20), span_of(3, 30), span_of(0, 40)};
    CHECK(build(tiny.data(), tiny.size(), g, &t, &why));
    CHECK(t.units.empty() && t.tails.size() == 6 && t.counts.columns == 6);
  }
  std::printf("ok   TestHandMade\n");
}

// The list's order on two small batches: object 0 of 16 one-vector-wide tiles (8 units of C = 2),
// object 1 of 4 tiles, object 2 empty -- three ticket groups in all.
void TestOrder() {
  const std::vector<Span> spans = {span_of(16 * 256, 0), span_of(4 * 256, 100000), span_of(0, 200000)};
  auto listed = [&](uint32_t segments) {
    Tables t;
    std::string why;
    CHECK(build(spans.data(), spans.size(), Geometry{1, 2, segments}, &t, &why));
    std::vector<std::pair<uint32_t, uint32_t>> out;
    for (const Unit& u : t.units) out.push_back({u.obj, u.tile});
    return out;
  };
  using L = std::vector<std::pair<uint32_t, uint32_t>>;
  // 64 segments wanted, 3 groups: segments of one group (8 tiles) -- object 0 is two segments.
  CHECK(listed(64) == (L{{0, 0}, {0, 2}, {0, 4}, {0, 6}, {0, 8}, {0, 10}, {0, 12}, {0, 14}, {1, 0}, {1, 2}}));
  // One segment wanted: every object is one segment, four units of each in turn.
  CHECK(listed(1) == (L{{0, 0}, {0, 2}, {0, 4}, {0, 6}, {1, 0}, {1, 2}, {0, 8}, {0, 10}, {0, 12}, {0, 14}}));
  // Two: segments of two groups, the same.
  CHECK(listed(2) == listed(1));
  std::printf("ok   TestOrder\n");
}

void TestRandom() {
  std::mt19937_64 rng(20240611);
  for (const Geometry g : geometries()) {
    const uint64_t T = 256ull * g.U;
    for (int round = 0; round < 200; ++round) {
      const size_t nobj = rng() % 40;
      std::vector<Span> spans;
      for (size_t o = 0; o < nobj; ++o) {
        uint64_t L;
        switch (rng() % 4) {
          case 0: L = rng() % 10; break;
          case 1: L = (rng() % 5) * T + rng() % 9; break;               // around tile boundaries
          case 2: L = (rng() % 4) * g.C * T + (rng() % 9) - 4 + 4; break;  // around unit boundaries
          default: L = rng() % (12 * T); break;
        }
        spans.push_back(Span{rng() % (1ull << 40), rng() % (1ull << 32), rng() % (1ull << 40), rng() % (1ull << 32), L});
      }
      check_tables(spans, g);
    }
  }
  std::printf("ok   TestRandom\n");
}

void TestRefusals() {
  for (const Geometry g : geometries()) {
    Counts c;
    std::string why;
    Span s = span_of(kMaxL - 1, 0);
    CHECK(count(&s, 1, g, &c, &why));  // the largest shard a batch takes
    CHECK(c.columns == kMaxL - 1 && c.tails == 3 && c.units == units_of(kMaxL - 1, g));
    s.L = kMaxL;  // 2^30
    why.clear();
    CHECK(!count(&s, 1, g, &c, &why) && why.find("2^30") != std::string::npos);
    Tables t;
    CHECK(!build(&s, 1, g, &t, &why));
    s.L = ~0ull;
    CHECK(!count(&s, 1, g, &c, &why));
    // A unit count of 2^32: the fewest largest objects that reach it are refused, one fewer is
    // counted (count() allocates nothing; the span list itself is a few hundred KB).
    const uint64_t per = units_of(kMaxL - 1, g);
    const uint64_t need = ((1ull << 32) + per - 1) / per;
    std::vector<Span> many(need, span_of(kMaxL - 1, 0));
    why.clear();
    CHECK(!count(many.data(), many.size(), g, &c, &why) && why.find("2^32") != std::string::npos);
    CHECK(count(many.data(), many.size() - 1, g, &c, &why));
    CHECK(c.units == (need - 1) * per && c.units < (1ull << 32));
    // The last unit below the bound: trim the last object so the count is exactly 2^32 - 1 ...
    const uint64_t T = 256ull * g.U, cut = need * per - ((1ull << 32) - 1);  // units to drop
    many.back().L = (per - cut) * g.C * T;
    CHECK(count(many.data(), many.size(), g, &c, &why) && c.units == (1ull << 32) - 1);
    // ... and one more column's vector tips it over.
    many.back().L += 4;
    CHECK(!count(many.data(), many.size(), g, &c, &why));
    // nobj itself is a 32-bit object index.
    CHECK(!count(nullptr, 1ull << 32, g, &c, &why));
  }
  std::printf("ok   TestRefusals\n");
}

}  // namespace

int main() {
  TestHandMade();
  TestOrder();
  TestRandom();
  TestRefusals();
  return 0;
}
