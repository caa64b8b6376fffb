// Host layout of a plan set (slime_rs_planset_create): several plans with the
// same k in ONE device table, so that a ragged launch can apply a different
// plan to every object (rs_ragged.hip, the planned kernels).  Pure host code,
// no HIP: tests/cpp/planset_table_test.cpp builds it with plain g++.
//
// The table is an array of 32-bit words:
//   records   one 64-byte Record per plan at word 16 * plan index, so a wave
//             takes a plan's record with one 16-dword scalar load from plan
//             index x record size.  A record holds the plan's row count and
//             the WORD offsets, from the table's start, of its three blocks;
//   blocks    per plan, in plan order: its k input shard indices, its `rows`
//             output shard indices and its coefficient rows.  The index blocks
//             are zero-padded to whole 16-word lines, so the k <= 16 kernels
//             take a plan's input indices with one 16-dword load; the
//             coefficient rows lie wide_coeff_stride(k) = ceil(k / 16) * 16
//             words apart (kCoeffStride for k <= 16), so load_coeff_row<K>
//             and wide_dot read them exactly as they read a plan's own table.
// Every record and every block starts on a 64-byte boundary of the table (the
// device allocation is aligned far beyond that).  Offsets are 32-bit: a set
// whose table would reach 2^32 words is refused.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace slime {
namespace planset {

// Plans of one set.  A planned batch stores a plan index per object in 32
// bits with 0xFFFFFFFF reserved; 2^20 patterns cover every erasure pattern of
// any code a repair sweep meets (12 choose 4 is 495) with a table that stays
// in the tens of megabytes.
constexpr uint32_t kMaxPlans = 1u << 20;
constexpr uint32_t kRecordWords = 16;

struct alignas(64) Record {
  uint32_t rows;       // output rows of the plan (>= 1)
  uint32_t in_off;     // word offset of its k input indices (one 16-word line per 16)
  uint32_t out_off;    // word offset of its `rows` output indices
  uint32_t coeff_off;  // word offset of its rows x row_stride(k) coefficients
  uint32_t in_max;     // its highest input / output shard index (host checks)
  uint32_t out_max;
  uint32_t reserved[10];  // zero
};
static_assert(sizeof(Record) == 4 * kRecordWords && alignof(Record) == 64, "one s_load_dwordx16 per record");

// One member plan as the caller holds it (host memory).
struct PlanView {
  uint32_t rows, k;
  const uint32_t* in_idx;   // k
  const uint32_t* out_idx;  // rows
  const uint32_t* coeff;    // rows x k, row-major, canonical residues
};

constexpr uint32_t pad16(uint32_t n) { return (n + 15u) & ~15u; }
// Words between a plan's coefficient rows (apply::wide_coeff_stride; apply::kCoeffStride for k <= 16).
constexpr uint32_t row_stride(uint32_t k) { return pad16(k); }

struct Table {
  uint32_t nplans = 0, k = 0;
  uint32_t max_rows = 0, in_max = 0, out_max = 0;  // over the set
  std::vector<uint32_t> words;
  Record record(uint32_t i) const {
    Record r;
    memcpy(&r, words.data() + (size_t)i * kRecordWords, sizeof r);
    return r;
  }
};

// false: *why names the refusal (no plans, more than kMaxPlans, a plan
// without rows or inputs, mixed k, a table of 2^32 words or more).
inline bool build(const PlanView* plans, uint64_t nplans, Table* t, std::string* why) {
  if (!plans || nplans == 0) {
    *why = "a plan set needs at least one plan";
    return false;
  }
  if (nplans > kMaxPlans) {
    *why = std::to_string(nplans) + " plans: a set holds at most " + std::to_string(kMaxPlans);
    return false;
  }
  const uint32_t k = plans[0].k;
  uint64_t total = nplans * kRecordWords;
  for (uint64_t i = 0; i < nplans; ++i) {
    const PlanView& p = plans[i];
    if (p.rows == 0 || p.k == 0 || !p.in_idx || !p.out_idx || !p.coeff) {
      *why = "plan " + std::to_string(i) + ": no rows or no inputs";
      return false;
    }
    if (p.k != k) {
      *why = "plan " + std::to_string(i) + " has k = " + std::to_string(p.k) + ", plan 0 has k = " + std::to_string(k) +
             " (the plans of a set share k)";
      return false;
    }
    total += (uint64_t)pad16(k) + pad16(p.rows) + (uint64_t)p.rows * row_stride(k);
    if (total >= (1ull << 32)) {
      *why = "the set's table would reach 2^32 words (split the set)";
      return false;
    }
  }
  t->nplans = (uint32_t)nplans;
  t->k = k;
  t->max_rows = t->in_max = t->out_max = 0;
  t->words.assign((size_t)total, 0u);
  uint32_t at = (uint32_t)nplans * kRecordWords;
  for (uint64_t i = 0; i < nplans; ++i) {
    const PlanView& p = plans[i];
    Record r{};
    r.rows = p.rows;
    r.in_off = at;
    r.out_off = r.in_off + pad16(k);
    r.coeff_off = r.out_off + pad16(p.rows);
    at = r.coeff_off + p.rows * row_stride(k);
    for (uint32_t j = 0; j < k; ++j) {
      t->words[r.in_off + j] = p.in_idx[j];
      if (p.in_idx[j] > r.in_max) r.in_max = p.in_idx[j];
    }
    for (uint32_t q = 0; q < p.rows; ++q) {
      t->words[r.out_off + q] = p.out_idx[q];
      if (p.out_idx[q] > r.out_max) r.out_max = p.out_idx[q];
      for (uint32_t j = 0; j < k; ++j) t->words[r.coeff_off + (size_t)q * row_stride(k) + j] = p.coeff[(size_t)q * k + j];
    }
    memcpy(t->words.data() + (size_t)i * kRecordWords, &r, sizeof r);
    if (p.rows > t->max_rows) t->max_rows = p.rows;
    if (r.in_max > t->in_max) t->in_max = r.in_max;
    if (r.out_max > t->out_max) t->out_max = r.out_max;
  }
  return true;
}

}  // namespace planset
}  // namespace slime
