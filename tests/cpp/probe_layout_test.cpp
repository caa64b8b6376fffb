// CPU test of the placement probe's layout (slime_amd/csrc/probe_layout.hpp):
// where placement_probe puts its objects and its coefficient / index table in
// a range of `bytes` bytes.  The kernels read the table with scalar loads,
// which ignore an address's low bits, so for EVERY byte count
//
//   - the table's offset is a multiple of 256 (so of 4),
//   - the table ends inside the range,
//   - the 128 objects of 12 shards of L symbols end at or before the table,
//   - L is a multiple of 64 (16-byte vectors from every shard base),
//
// over every bytes % 256 residue at several sizes, around the smallest size
// the probe accepts (~402 MB), around 512 MiB and 16 GiB +- 3, and the
// refusals (too small: L == 0).
// Usage: probe_layout_test   (exit 0 = pass)
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "probe_layout.hpp"

using namespace slime::probe;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

namespace {

constexpr uint64_t kObjBytesPerL = 4ull * kTotal * kObj;  // bytes of the walk per symbol of L

// The invariants of an accepted layout.
void check_accepted(uint64_t bytes) {
  const Layout l = layout(bytes);
  CHECK(l.L >= kMinL);
  CHECK(l.L % 64 == 0);
  CHECK(l.table_off % 256 == 0);
  CHECK(l.table_off + 4ull * kTableWords <= bytes);
  CHECK(kObjBytesPerL * l.L <= l.table_off);
  // The table keeps to the range's last 4 KiB + one 256-byte step, and the
  // walk uses all the room 64-symbol granularity allows.
  CHECK(bytes - l.table_off >= kTableRoom && bytes - l.table_off < kTableRoom + 256);
  CHECK(kObjBytesPerL * (l.L + 64) > l.table_off);
}

// The smallest accepted byte count: kMinL symbols of walk, then the table's room.
constexpr uint64_t kSmallest = kObjBytesPerL * kMinL + kTableRoom;

void TestEveryResidue() {
  const uint64_t bases[] = {kSmallest, 512ull << 20, (1ull << 32) - 256, 1ull << 32, 16ull << 30, 200ull << 30};
  for (uint64_t b : bases)
    for (uint64_t r = 0; r < 256; ++r) check_accepted(b + r);
  // A multiple of 256 keeps the table where it has always been: bytes - 4096.
  for (uint64_t b : bases) CHECK(layout(b).table_off == b - kTableRoom);
  std::printf("ok   TestEveryResidue\n");
}

void TestAroundTheSizesCallersUse() {
  // 402 MB: the smallest probed size; 512 MiB + 1: an odd torch uint8 tensor;
  // 16 GiB: where device_alloc starts to probe, and device_empty(uint8, odd).
  const uint64_t mids[] = {kSmallest + 3, 512ull << 20, 16ull << 30};
  for (uint64_t m : mids)
    for (uint64_t b = m - 3; b <= m + 3; ++b) check_accepted(b);
  CHECK(kSmallest == 402657280ull);  // the "~400 MB" of include/slime_rs.h
  CHECK(layout(kSmallest).L == kMinL);
  CHECK(layout((512ull << 20) + 1).table_off == (512ull << 20) - kTableRoom);
  CHECK(layout((16ull << 30) + 3).table_off == (16ull << 30) - kTableRoom);
  CHECK(layout((16ull << 30) - 3).table_off == (16ull << 30) - kTableRoom - 256);
  std::printf("ok   TestAroundTheSizesCallersUse\n");
}

void TestRefusals() {
  const uint64_t small[] = {0, 1, 3, 4095, 4096, 8191, 8192, 8193, 1ull << 20, kSmallest - 256, kSmallest - 1};
  for (uint64_t b : small) CHECK(layout(b).L == 0);
  // Under the smallest size every residue is refused, at it every one accepted.
  for (uint64_t r = 1; r <= 256; ++r) CHECK(layout(kSmallest - r).L == 0);
  CHECK(layout(kSmallest).L == kMinL);
  std::printf("ok   TestRefusals\n");
}

}  // namespace

int main() {
  TestEveryResidue();
  TestAroundTheSizesCallersUse();
  TestRefusals();
  return 0;
}
