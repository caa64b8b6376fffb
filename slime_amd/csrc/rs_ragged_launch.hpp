// Host side of the ragged launches (rs_ragged.hip, rs_verify_ragged.hip,
// rs_bytes_ragged.hip, rs_bytes_ragged_encode.hip): the grid of a launch, the
// compile-time k, the choice between the three schedules and verify's row
// blocks, each written once.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.hpp"
#include "rs_apply_kernel.hpp"  // apply::kBlock

namespace slime {
namespace ragged {

constexpr uint64_t kQueueBlocks = 256;  // one block per CU, as launch_queue (rs_apply.hip)

// Blocks of a ragged launch: one wave per unit up to `full` (queue_blocks),
// and enough lanes for the per-lane items after the walk (the tail list; the
// byte encode's edge columns) of a batch of many short objects.
inline uint64_t ragged_blocks(uint64_t full, uint64_t nunits, uint64_t nitems) {
  const uint64_t by_units = queue_blocks(full, nunits);
  const uint64_t by_items = (nitems + apply::kBlock - 1) / apply::kBlock;
  const uint64_t want = by_items < full ? by_items : full;
  return by_units > want ? by_units : want;
}

// f(std::integral_constant<int, K>) for a launch's k in 1 ... 16.
template <class F>
hipError_t with_k(uint32_t k, F&& f) {
  switch (k) {
#define SLIME_K(n) \
  case n: return f(std::integral_constant<int, n>{});
    SLIME_K(1) SLIME_K(2) SLIME_K(3) SLIME_K(4) SLIME_K(5) SLIME_K(6) SLIME_K(7) SLIME_K(8)
    SLIME_K(9) SLIME_K(10) SLIME_K(11) SLIME_K(12) SLIME_K(13) SLIME_K(14) SLIME_K(15)
#undef SLIME_K
    default: return f(std::integral_constant<int, 16>{});
  }
}

// The choice between the schedules of a vector (k <= 16) launch over `nunits`
// units and `nitems` per-lane items.  launch(dyn, pipe, blocks, ticket) starts
// the kernel's <DYN, PIPE> form (two std::bool_constant) on `blocks` blocks
// and returns hipGetLastError():
//   slime_rs_kernel_pipeline(0): static, one tile at a time;
//   the stream may take the dynamic schedule and there is more than one
//     block's units to balance (queue_spread, kernels.hpp): tickets from a
//     counter set, one block a CU;
//   otherwise -- schedule mode 0, a capture under mode 1, no counter set to be
//     had -- static, double-buffered.
// static_full: the block budget of the two static forms.
template <class Launch>
hipError_t launch_scheduled(hipStream_t s, uint32_t nunits, uint64_t nitems, uint64_t static_full, Launch&& launch) {
  const uint64_t static_blocks = ragged_blocks(static_full, nunits, nitems);
  if (!pipelined_kernels()) return launch(std::false_type{}, std::false_type{}, static_blocks, (uint32_t*)nullptr);
  if (queue_allowed(s) && nunits > tiny_queue_units()) {
    bool launched = false;
    const uint64_t blocks = ragged_blocks(kQueueBlocks, nunits, nitems);
    const hipError_t e = with_tickets(
        s, [&](uint32_t* set) { return launch(std::true_type{}, std::true_type{}, blocks, set); }, &launched);
    if (launched || e != hipSuccess) return e;
  }
  return launch(std::false_type{}, std::true_type{}, static_blocks, (uint32_t*)nullptr);
}

// One row block [r0, r0 + rows_c) of a verify launch `v`.  A launch tallies at
// most 64 rows (one lane each): larger plans and sets go in row blocks, f(block)
// for each in turn.  Single plan: the kernel is given the plan's pointers moved
// on to the block; set: the table and r0.
template <class V>
struct RowBlock {
  const V& v;
  uint32_t r0, rows_c;
};
template <class V, class F>
hipError_t for_row_blocks(const V& v, F&& f) {
  for (uint32_t r0 = 0; r0 < v.p.rows; r0 += 64) {
    const RowBlock<V> b{v, r0, v.p.rows - r0 < 64 ? v.p.rows - r0 : 64};
    if (hipError_t e = f(b)) return e;
  }
  return hipSuccess;
}

}  // namespace ragged
}  // namespace slime
