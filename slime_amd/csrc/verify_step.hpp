// How the ragged verify kernels (rs_verify_ragged.hip) take a batch tile.
// Pure host code, no HIP: tests/cpp/verify_step_test.cpp builds it with g++.
//
// A batch's tile is 64 U 16-byte vectors of every shard, U = unroll_for_k(k)
// vectors a lane (ragged_plan.hpp): the apply launch's value, a function of k
// alone because one batch serves execute and verify.  Verify holds k inputs
// AND R stored rows per vector (R = 2 for plans of up to two rows, else 4),
// twice in the double-buffered loop, so its budget is smaller than apply's:
//   budget(k, R) = 24 / (k + R) vectors a lane, clipped to 1 ... 4
// -- the uniform verify launch's unroll (rs_verify.hip, verify_unroll_c).  A
// wave therefore takes a tile in steps(k, R) = ceil(U / budget) steps of
//   width(k, R) = ceil(U / steps) <= budget
// vectors a lane each, the last one clipped to the tile's (and the object's)
// end: U = 4 under a budget of 3 goes 2 + 2, not 3 + 1; U = 3 under a budget
// of 2 goes 2 + 1 (the steps need not divide the tile evenly).  The software
// pipeline runs over steps, not tiles.
#pragma once
#include <stdint.h>

#include "ragged_plan.hpp"

namespace slime {
namespace verify_step {

constexpr int kVectorBudget = 24;  // 16-byte vectors a lane holds per pipeline stage

// Stored rows that travel with a step's inputs, by the launch's row count.
constexpr int stored_rows(uint32_t rows) { return rows <= 2 ? 2 : 4; }

constexpr int budget(int k, int R) {
  return kVectorBudget / (k + R) > 4 ? 4 : kVectorBudget / (k + R) < 1 ? 1 : kVectorBudget / (k + R);
}
constexpr int steps(int k, int R) {
  return (ragged::unroll_for_k(k) + budget(k, R) - 1) / budget(k, R);
}
constexpr int width(int k, int R) {
  return (ragged::unroll_for_k(k) + steps(k, R) - 1) / steps(k, R);
}

// Step s of a tile that holds `nvec` vectors (1 ... 64 U; an object's last
// tile may hold fewer than 64 U): vectors [first, first + count) of the tile.
// count == 0: the tile has no step s (it ended before).
struct Step {
  uint32_t first, count;
};
constexpr Step step_of(int k, int R, uint32_t nvec, uint32_t s) {
  const uint32_t w = 64u * (uint32_t)width(k, R);
  const uint32_t a = s * w < nvec ? s * w : nvec;
  const uint32_t b = a + w < nvec ? a + w : nvec;
  return Step{a, b - a};
}
// Steps a tile of `nvec` vectors takes: ceil(nvec / (64 width)).
constexpr uint32_t steps_of(int k, int R, uint32_t nvec) {
  return (nvec + 64u * (uint32_t)width(k, R) - 1) / (64u * (uint32_t)width(k, R));
}

}  // namespace verify_step
}  // namespace slime
