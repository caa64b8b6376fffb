// Where the placement probe (device_alloc.cpp: placement_probe) puts its
// objects and its coefficient / index table inside a caller's byte range.
// Pure arithmetic, so that tests/cpp/probe_layout_test.cpp checks it on the
// CPU for every size class.
//
// The probe walks kObj objects of kTotal shards of L symbols from the start of
// the range and keeps its table behind them, in the range's last 4 KiB.  The
// kernels read the table with scalar loads, which ignore an address's low two
// bits: the table's offset must be a multiple of 4 for ANY byte count (a range
// of 4n+1 bytes is legal), or the shard indices come out shifted and the walk
// leaves the range.  The offset is rounded down to 256 bytes, so the table
// also starts on a cache line.
#pragma once
#include <cstdint>

namespace slime {
namespace probe {

constexpr uint32_t kNeed = 8, kTotal = 12, kRows = kTotal - kNeed, kObj = 128;
// kRows coefficient rows of 16 words, then 8 input and 8 output shard indices.
constexpr uint32_t kTableWords = kRows * 16 + 16;
constexpr uint64_t kTableRoom = 4096;  // the range's tail kept for the table
constexpr uint64_t kMinL = 65536;      // below this the walk is too short to time

struct Layout {
  uint64_t table_off = 0;  // byte offset of the table from the range's start, a multiple of 256
  uint64_t L = 0;          // symbols per shard, a multiple of 64; 0: range too small, no probe
};

// The layout for a range of `bytes` bytes (L == 0: too small to measure).
//   table_off + 4*kTableWords <= bytes        (the table is inside the range)
//   kTotal*kObj*L*4 <= table_off              (the objects end before the table)
inline Layout layout(uint64_t bytes) {
  Layout r;
  if (bytes < 2 * kTableRoom) return r;
  r.table_off = (bytes - kTableRoom) & ~(uint64_t)255;
  const uint64_t L = (r.table_off / 4 / kTotal / kObj) & ~(uint64_t)63;
  if (L >= kMinL) r.L = L;
  return r;
}

}  // namespace probe
}  // namespace slime
