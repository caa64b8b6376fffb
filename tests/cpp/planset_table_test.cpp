// CPU test of a plan set's host layout (slime_amd/csrc/planset_table.hpp) and
// of the planned form of a ragged batch's work tables (ragged_plan.hpp with
// plan_of), the tables slime_rs_planset_create and
// slime_rs_batch_create_planned upload and the planned kernels of
// rs_ragged.hip read.
//
//   - seeded random sets, k from 1 to 40, rows from 1 to 8: every record and
//     every block starts on a 64-byte boundary inside the buffer, blocks do not
//     overlap, and every record round-trips to its plan's rows, indices and
//     coefficients at the strides the row-load idioms use (one 16-word line of
//     input indices for k <= 16, coefficient rows ceil(k / 16) * 16 words
//     apart), padding zero, set-wide maxima right;
//   - refusals: mixed k, zero plans, above the bound, a plan without rows;
//   - planned batch tables: the descriptor carries the index; NO_PLAN objects
//     and L == 0 objects yield no unit and no tail; the unit and tail lists
//     otherwise equal the unplanned build's over the remaining objects;
//     plan_of[o] >= nplans is refused; without plan_of nothing changed.
// Usage: planset_table_test   (exit 0 = pass)
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "planset_table.hpp"
#include "ragged_plan.hpp"

using namespace slime;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

namespace {

struct HostPlan {
  uint32_t rows, k;
  std::vector<uint32_t> in_idx, out_idx, coeff;
  planset::PlanView view() const { return planset::PlanView{rows, k, in_idx.data(), out_idx.data(), coeff.data()}; }
};

HostPlan random_plan(std::mt19937_64& rng, uint32_t k, uint32_t rows) {
  HostPlan p{rows, k, {}, {}, {}};
  for (uint32_t j = 0; j < k; ++j) p.in_idx.push_back((uint32_t)(rng() % 200));
  for (uint32_t i = 0; i < rows; ++i) p.out_idx.push_back((uint32_t)(rng() % 200));
  for (uint32_t i = 0; i < rows * k; ++i) p.coeff.push_back((uint32_t)(rng() % 4294967291ull));
  return p;
}

void TestRandomSets() {
  std::mt19937_64 rng(20260);
  for (uint32_t k = 1; k <= 40; ++k) {
    const uint32_t nplans = 1 + (uint32_t)(rng() % 9);
    std::vector<HostPlan> plans;
    std::vector<planset::PlanView> views;
    for (uint32_t i = 0; i < nplans; ++i) plans.push_back(random_plan(rng, k, 1 + (i + k) % 8));  // rows 1..8
    for (const HostPlan& p : plans) views.push_back(p.view());
    planset::Table t;
    std::string why;
    CHECK(planset::build(views.data(), views.size(), &t, &why));
    CHECK(t.nplans == nplans && t.k == k);
    const uint64_t n = t.words.size();
    const uint32_t stride = (k + 15) / 16 * 16;
    CHECK(planset::row_stride(k) == stride);
    std::vector<char> used(n, 0);
    auto claim = [&](uint64_t at, uint64_t len) {
      CHECK(at % 16 == 0);  // 64-byte boundary
      CHECK(at + len <= n);
      for (uint64_t q = at; q < at + len; ++q) {
        CHECK(!used[q]);
        used[q] = 1;
      }
    };
    uint32_t max_rows = 0, in_max = 0, out_max = 0;
    for (uint32_t i = 0; i < nplans; ++i) {
      const HostPlan& p = plans[i];
      claim((uint64_t)i * planset::kRecordWords, planset::kRecordWords);  // the record: plan index x record size
      const planset::Record r = t.record(i);
      CHECK(r.rows == p.rows);
      claim(r.in_off, planset::pad16(k));
      claim(r.out_off, planset::pad16(p.rows));
      claim(r.coeff_off, (uint64_t)p.rows * stride);
      uint32_t pin = 0, pout = 0;
      for (uint32_t j = 0; j < planset::pad16(k); ++j) CHECK(t.words[r.in_off + j] == (j < k ? p.in_idx[j] : 0u));
      for (uint32_t q = 0; q < planset::pad16(p.rows); ++q) CHECK(t.words[r.out_off + q] == (q < p.rows ? p.out_idx[q] : 0u));
      for (uint32_t q = 0; q < p.rows; ++q)
        for (uint32_t j = 0; j < stride; ++j)
          CHECK(t.words[r.coeff_off + (uint64_t)q * stride + j] == (j < k ? p.coeff[(size_t)q * k + j] : 0u));
      for (uint32_t v : p.in_idx) pin = v > pin ? v : pin;
      for (uint32_t v : p.out_idx) pout = v > pout ? v : pout;
      CHECK(r.in_max == pin && r.out_max == pout);
      for (uint32_t v : r.reserved) CHECK(v == 0);
      max_rows = p.rows > max_rows ? p.rows : max_rows;
      in_max = pin > in_max ? pin : in_max;
      out_max = pout > out_max ? pout : out_max;
    }
    for (uint64_t q = 0; q < n; ++q) CHECK(used[q]);  // nothing but records and blocks
    CHECK(t.max_rows == max_rows && t.in_max == in_max && t.out_max == out_max);
  }
  std::printf("ok   TestRandomSets\n");
}

void TestSetRefusals() {
  std::mt19937_64 rng(7);
  const HostPlan a = random_plan(rng, 8, 4), b = random_plan(rng, 7, 2);
  planset::Table t;
  std::string why;
  const planset::PlanView mixed[2] = {a.view(), b.view()};
  CHECK(!planset::build(mixed, 2, &t, &why) && why.find("share k") != std::string::npos);
  CHECK(!planset::build(mixed, 0, &t, &why) && why.find("at least one") != std::string::npos);
  CHECK(!planset::build(nullptr, 3, &t, &why));
  // Above the bound: refused on the count alone, the array is never read.
  CHECK(planset::kMaxPlans >= 65536);
  CHECK(!planset::build(mixed, (uint64_t)planset::kMaxPlans + 1, &t, &why) && why.find("at most") != std::string::npos);
  planset::PlanView norows = a.view();
  norows.rows = 0;
  CHECK(!planset::build(&norows, 1, &t, &why));
  // The bound itself is accepted: 65536 one-row plans.
  const HostPlan one = random_plan(rng, 3, 1);
  std::vector<planset::PlanView> many(65536, one.view());
  CHECK(planset::build(many.data(), many.size(), &t, &why));
  CHECK(t.nplans == 65536 && t.record(65535).rows == 1);
  std::printf("ok   TestSetRefusals\n");
}

void TestPlannedBatch() {
  std::mt19937_64 rng(99);
  for (int k : {1, 3, 4, 8, 12, 16, 17, 40}) {
    const ragged::Geometry g = ragged::geometry_for_k(k);
    const uint64_t T = 256ull * g.U;
    for (int round = 0; round < 6; ++round) {
      const uint32_t nplans = 1 + (uint32_t)(rng() % 5);
      std::vector<ragged::Span> spans;
      std::vector<uint32_t> plan_of;
      const uint64_t lens[] = {0, 1, 3, 4, 5, 255, 257, T - 1, T, T + 1, g.C * T + 1, 4 * g.C * T + 5, 9 * g.C * T};
      const size_t nobj = 5 + rng() % 40;
      for (size_t o = 0; o < nobj; ++o) {
        const uint64_t L = lens[rng() % (sizeof lens / sizeof *lens)];
        spans.push_back(ragged::Span{o * 1000, L + 3, o * 2000 + 1, L + 7, L});
        plan_of.push_back(rng() % 3 == 0 ? ragged::kNoPlan : (uint32_t)(rng() % nplans));
      }
      ragged::Tables t;
      std::string why;
      CHECK(ragged::build(spans.data(), nobj, g, &t, &why, plan_of.data(), nplans));
      // The unplanned build over the remaining objects.
      std::vector<ragged::Span> rest;
      std::vector<uint32_t> orig;
      for (size_t o = 0; o < nobj; ++o)
        if (plan_of[o] != ragged::kNoPlan) {
          rest.push_back(spans[o]);
          orig.push_back((uint32_t)o);
        }
      ragged::Tables u;
      CHECK(ragged::build(rest.data(), rest.size(), g, &u, &why));
      CHECK(t.units.size() == u.units.size() && t.tails.size() == u.tails.size());
      for (size_t q = 0; q < u.units.size(); ++q)
        CHECK(t.units[q].obj == orig[u.units[q].obj] && t.units[q].tile == u.units[q].tile);
      for (size_t q = 0; q < u.tails.size(); ++q)
        CHECK(t.tails[q].obj == orig[u.tails[q].obj] && t.tails[q].col == u.tails[q].col);
      CHECK(t.counts.units == u.counts.units && t.counts.tails == u.counts.tails &&
            t.counts.columns == u.counts.columns && t.counts.tiles == u.counts.tiles && t.counts.nobj == nobj);
      // Descriptors: the index, and nothing to do for NO_PLAN and empty objects.
      CHECK(t.desc.size() == nobj);
      for (size_t o = 0; o < nobj; ++o) {
        const ragged::Desc& d = t.desc[o];
        CHECK(d.reserved[0] == plan_of[o]);
        for (int q = 1; q < 5; ++q) CHECK(d.reserved[q] == 0);
        CHECK(d.src_off == spans[o].src_off && d.dst_off == spans[o].dst_off);
        CHECK(d.src_shard == spans[o].src_shard_stride && d.dst_shard == spans[o].dst_shard_stride);
        const uint64_t L = plan_of[o] == ragged::kNoPlan ? 0 : spans[o].L;
        CHECK(d.ncols == L && d.nvec == L / 4 && d.ntiles == ragged::tiles_of(L, g.U));
      }
      for (const ragged::Unit& un : t.units) CHECK(plan_of[un.obj] != ragged::kNoPlan && spans[un.obj].L >= 4);
      for (const ragged::Tail& ta : t.tails) CHECK(plan_of[ta.obj] != ragged::kNoPlan && spans[ta.obj].L != 0);
      // An index at or past nplans is refused, by count() already.
      std::vector<uint32_t> bad = plan_of;
      bad[nobj / 2] = nplans;
      ragged::Counts c;
      CHECK(!ragged::count(spans.data(), nobj, g, &c, &why, bad.data(), nplans));
      CHECK(why.find("plan index") != std::string::npos && why.find("span " + std::to_string(nobj / 2)) != std::string::npos);
      CHECK(!ragged::build(spans.data(), nobj, g, &t, &why, bad.data(), nplans));
      // Without plan_of the reserved words stay zero.
      CHECK(ragged::build(spans.data(), nobj, g, &t, &why));
      for (const ragged::Desc& d : t.desc)
        for (uint32_t v : d.reserved) CHECK(v == 0);
    }
  }
  // A NO_PLAN object's length is still validated.
  const ragged::Span big{0, 1, 0, 1, ragged::kMaxL};
  const uint32_t none = ragged::kNoPlan;
  ragged::Counts c;
  std::string why;
  CHECK(!ragged::count(&big, 1, ragged::geometry_for_k(8), &c, &why, &none, 1));
  std::printf("ok   TestPlannedBatch\n");
}

}  // namespace

int main() {
  TestRandomSets();
  TestSetRefusals();
  TestPlannedBatch();
  std::printf("planset_table_test: all passed\n");
  return 0;
}
