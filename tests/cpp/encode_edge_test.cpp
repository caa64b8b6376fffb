// The ragged byte encode's edge geometry (encode_edge.hpp) against a brute-force
// classification of every word, CPU only:
//   for every k <= 20 and every S up to 4k * 70, with L = ceil(ceil(S/4) / k):
//   - no column below 4 * interior holds a partial or padding word in any data chunk,
//   - the first column at or past the bound is needed (the bound is not loose by a vector),
//   - at most k + 3 columns lie at or past the bound,
//   - nw and tailmask are the object's;
//   and for sizes that contradict L, the clamp: nw <= kL and interior <= L / 4.
#include <cstdint>
#include <cstdio>

#include "encode_edge.hpp"

using slime::edge::Geom;
using slime::edge::geom;

static int fails = 0;
#define CHECK(c, ...)                  \
  do {                                 \
    if (!(c)) {                        \
      if (++fails <= 20) {             \
        std::printf("FAIL %s: ", #c);  \
        std::printf(__VA_ARGS__);      \
        std::printf("\n");             \
      }                                \
    }                                  \
  } while (0)

// Word w of an object of S bytes: 0 whole, 1 partial, 2 padding.
static int classify(uint64_t w, uint64_t S) {
  if (4 * w + 4 <= S) return 0;
  return 4 * w < S ? 1 : 2;
}

int main() {
  uint64_t cases = 0, most = 0;
  for (uint32_t k = 1; k <= 20; ++k) {
    for (uint64_t S = 0; S <= 4ull * k * 70; ++S) {
      const uint64_t nw = (S + 3) / 4, L = (nw + k - 1) / k;
      const Geom g = geom(S, L, k);
      ++cases;
      CHECK(g.nw == nw, "k=%u S=%llu nw=%llu", k, (unsigned long long)S, (unsigned long long)g.nw);
      const uint32_t mask = S % 4 ? 0xFFFFFFFFu << (8 * (4 - S % 4)) : 0xFFFFFFFFu;
      CHECK(g.tailmask == mask, "k=%u S=%llu mask=%08x", k, (unsigned long long)S, g.tailmask);
      CHECK(4ull * g.interior <= L, "k=%u S=%llu interior=%u L=%llu", k, (unsigned long long)S, g.interior,
            (unsigned long long)L);
      for (uint64_t c = 0; c < 4ull * g.interior; ++c)
        for (uint32_t j = 0; j < k; ++j)
          CHECK(classify(j * L + c, S) == 0, "k=%u S=%llu column %llu chunk %u below the bound is not whole", k,
                (unsigned long long)S, (unsigned long long)c, j);
      // The vector at the bound, if the chunk has one, holds a word that is not whole.
      if (4ull * g.interior + 4 <= L) {
        bool edge = false;
        for (uint64_t c = 4ull * g.interior; c < 4ull * g.interior + 4; ++c)
          for (uint32_t j = 0; j < k; ++j) edge = edge || classify(j * L + c, S) != 0;
        CHECK(edge, "k=%u S=%llu the vector at the bound is interior", k, (unsigned long long)S);
      }
      const uint64_t ncol = L - 4ull * g.interior;
      CHECK(ncol <= slime::edge::edge_columns_max(k), "k=%u S=%llu %llu edge columns", k, (unsigned long long)S,
            (unsigned long long)ncol);
      if (ncol > most) most = ncol;
    }
    // Sizes that contradict L: clamped, never past the object's own chunks.
    for (uint64_t L = 0; L <= 9; ++L)
      for (uint64_t S = 0; S <= 4ull * k * 12; ++S) {
        const Geom g = geom(S, L, k);
        ++cases;
        CHECK(g.nw <= (uint64_t)k * L, "k=%u L=%llu S=%llu nw=%llu", k, (unsigned long long)L, (unsigned long long)S,
              (unsigned long long)g.nw);
        CHECK(4ull * g.interior <= L, "k=%u L=%llu S=%llu interior=%u", k, (unsigned long long)L,
              (unsigned long long)S, g.interior);
        for (uint64_t c = 0; c < 4ull * g.interior; ++c)
          for (uint32_t j = 0; j < k; ++j)
            CHECK(classify(j * L + c, S) == 0, "k=%u L=%llu S=%llu column %llu chunk %u", k, (unsigned long long)L,
                  (unsigned long long)S, (unsigned long long)c, j);
      }
  }
  if (fails) {
    std::printf("encode_edge_test: %d failures\n", fails);
    return 1;
  }
  std::printf("encode_edge_test ok: %llu cases, at most %llu edge columns\n", (unsigned long long)cases,
              (unsigned long long)most);
  return 0;
}
