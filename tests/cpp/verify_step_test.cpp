// The ragged verify's step rule (verify_step.hpp), CPU only: for every k of the
// vector kernels and both stored-row counts, the steps of a batch tile cover
// the tile's vectors exactly once and in order, and no step holds more vectors
// a lane than the budget the rule states.
#include <stdio.h>
#include <stdlib.h>

#include "verify_step.hpp"

using namespace slime;

static int failures = 0;
#define CHECK(c, ...)              \
  do {                             \
    if (!(c)) {                    \
      ++failures;                  \
      fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");       \
    }                              \
  } while (0)

// The budget as the issue states it, restated: 24 / (k + R) clipped to 1..4.
static int stated_budget(int k, int R) {
  int b = 24 / (k + R);
  if (b > 4) b = 4;
  if (b < 1) b = 1;
  return b;
}

int main() {
  static_assert(verify_step::stored_rows(1) == 2 && verify_step::stored_rows(2) == 2 &&
                    verify_step::stored_rows(3) == 4 && verify_step::stored_rows(64) == 4,
                "R = 2 for plans of up to two rows, else 4");
  // The cases the design names.
  static_assert(verify_step::width(8, 4) == 2 && verify_step::steps(8, 4) == 2, "8/12: apply's 3 as 2 + 1");
  static_assert(verify_step::width(3, 2) == 4 && verify_step::steps(3, 2) == 1, "3/5: the whole tile");
  static_assert(verify_step::width(4, 4) == 2 && verify_step::steps(4, 4) == 2, "4/8: 2 + 2, not 3 + 1");
  static_assert(verify_step::width(10, 4) == 1 && verify_step::steps(10, 4) == 3, "10/14: 1 + 1 + 1");
  static_assert(verify_step::width(16, 4) == 1 && verify_step::steps(16, 4) == 1, "16/20: the tile is one vector");
  for (int k = 1; k <= 16; ++k) {
    const int U = ragged::unroll_for_k(k);
    const uint32_t tile = 64u * (uint32_t)U;
    for (int R : {2, 4}) {
      const int W = verify_step::width(k, R), S = verify_step::steps(k, R), B = verify_step::budget(k, R);
      CHECK(B == stated_budget(k, R), "k %d R %d: budget %d", k, R, B);
      CHECK(W >= 1 && W <= B && W <= U, "k %d R %d: width %d budget %d U %d", k, R, W, B, U);
      CHECK(S * W >= U && (S - 1) * W < U, "k %d R %d: %d steps of %d for U %d", k, R, S, W, U);
      // every tile size an object's last tile may have, and the whole tile
      for (uint32_t nvec = 1; nvec <= tile; ++nvec) {
        const uint32_t ns = verify_step::steps_of(k, R, nvec);
        CHECK(ns >= 1 && ns <= (uint32_t)S, "k %d R %d nvec %u: %u steps", k, R, nvec, ns);
        uint32_t at = 0;
        for (uint32_t s = 0; s < ns; ++s) {
          const verify_step::Step st = verify_step::step_of(k, R, nvec, s);
          CHECK(st.first == at, "k %d R %d nvec %u step %u starts at %u, not %u", k, R, nvec, s, st.first, at);
          CHECK(st.count >= 1 && st.count <= 64u * (uint32_t)B, "k %d R %d nvec %u step %u holds %u vectors", k, R,
                nvec, s, st.count);
          CHECK(s + 1 == ns || st.count == 64u * (uint32_t)W, "k %d R %d nvec %u: only the last step is short", k, R,
                nvec);
          at += st.count;
        }
        CHECK(at == nvec, "k %d R %d nvec %u: steps cover %u", k, R, nvec, at);
        // past the last step: nothing
        CHECK(verify_step::step_of(k, R, nvec, ns).count == 0, "k %d R %d nvec %u: a step past the end", k, R, nvec);
      }
      CHECK(verify_step::steps_of(k, R, tile) == (uint32_t)S, "k %d R %d: a whole tile takes %d steps", k, R, S);
    }
  }
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("verify_step_test ok\n");
  return 0;
}
