// fold96 (slime_amd/csrc/gfp.hpp, __host__ __device__) on the CPU against
// unsigned __int128 % p.  Random 96-bit values take its two rare branches
// (`u >> 32 == 1`, the final `w >= p`) with probability about 2^-30 each, so
// the values are built: multiples of p plus a small residue and values a small
// step below a power of 2^32, around every limb boundary and for every wrap
// count hi a 112-term sum can reach and beyond; the matrix-core range (hi = 0,
// lo < 2^49); every combination of edge limbs; then random values.
// Exit status 0 = every value folds to V mod p and both rare branches were taken.
#include <stdint.h>
#include <stdio.h>

#include <random>

// gfp.hpp is HIP code; its host fold96 compiles as plain C++ with these.
#define __host__
#define __device__
#define __forceinline__ inline
#include "gfp.hpp"

using namespace slime;
typedef unsigned __int128 u128;

static uint64_t g_n = 0, g_ubranch = 0, g_wbranch = 0, g_th[32] = {0};

// The fold's steps restated, only to count which branches the values reach.
static void count_branches(uint64_t lo, uint32_t hi) {
  const uint64_t t = (lo >> 32) * 5u + (uint32_t)lo + (uint64_t)hi * 25u;
  const uint64_t u = (t >> 32) * 5u + (uint32_t)t;
  const uint32_t w = (uint32_t)u + (uint32_t)(u >> 32) * 5u;
  if (hi <= 300) ++g_th[(t >> 32) & 31];
  g_ubranch += u >> 32 == 1;
  g_wbranch += w >= kP;
}

static bool check(u128 V) {
  const uint64_t lo = (uint64_t)V;
  const uint32_t hi = (uint32_t)(V >> 64);
  const uint32_t got = fold96(lo, hi), want = (uint32_t)(V % kP);
  ++g_n;
  count_branches(lo, hi);
  if (got != want) {
    fprintf(stderr, "MISMATCH fold96(lo=0x%016llx, hi=%u) = %u, want %u\n", (unsigned long long)lo, hi, got, want);
    return false;
  }
  return true;
}

int main() {
  const u128 one = 1;
  // Around every limb boundary of every wrap count: V = q p + t and V = q 2^32 + t - d.
  for (uint32_t hi = 0; hi <= 300; ++hi) {
    const u128 H = (u128)hi << 64;
    const u128 bases[] = {H,
                          H + (one << 32),
                          H + (one << 33),
                          H + (one << 63),
                          H + (one << 64) - (one << 33),
                          H + (one << 64) - (one << 32),
                          H + (one << 64)};
    for (u128 B : bases) {
      const u128 qp = B / kP, q32 = B >> 32;
      for (int dq = -2; dq <= 2; ++dq) {
        if ((dq < 0 && qp < (u128)(-dq)) || (dq < 0 && q32 < (u128)(-dq))) continue;
        for (uint32_t t = 0; t <= 44; ++t) {
          const u128 V = (qp + dq) * kP + t;
          if (V >> 64 <= 300 && !check(V)) return 1;
          for (uint32_t d = 0; d <= 44; ++d) {
            const u128 W = ((q32 + dq) << 32) + t;
            if (W >= d && (W - d) >> 64 <= 300 && !check(W - d)) return 1;
          }
        }
      }
    }
  }
  // The matrix-core paths fold rowc + v with hi = 0: lo < 2^49.
  {
    const uint64_t top = 1ull << 49;
    for (uint64_t q = 0; q * kP < top; q += 1 + (q >> 4)) {  // every q at first, then ever sparser
      for (uint32_t t = 0; t <= 44; ++t)
        if (q * kP + t < top && !check(q * kP + t)) return 1;
      if (q && !check(q * kP - 1)) return 1;
    }
    for (uint64_t m = 0; m < (1u << 17); m += 1 + (m >> 6))
      for (uint32_t d = 0; d <= 44; ++d) {
        if (m && !check((m << 32) - d)) return 1;
        if (!check((m << 32) + d)) return 1;
      }
    for (uint32_t d = 1; d <= 44; ++d)
      if (!check(top - d)) return 1;
    std::mt19937_64 rng(49);
    for (int i = 0; i < 1000000; ++i)
      if (!check(rng() >> 15)) return 1;
  }
  // Every (lo, hi) whose three limbs are edge values.
  {
    uint32_t limb[10] = {0u, 1u, 4u, 5u};
    for (uint32_t i = 0; i < 6; ++i) limb[4 + i] = 0xFFFFFFFAu + i;
    for (uint32_t h : limb)
      for (uint32_t m : limb)
        for (uint32_t l : limb)
          if (!check(((u128)h << 64) | ((u128)m << 32) | l)) return 1;
  }
  if (!g_ubranch || !g_wbranch) {
    fprintf(stderr, "the built values never took a rare branch (u: %llu, w: %llu)\n", (unsigned long long)g_ubranch,
            (unsigned long long)g_wbranch);
    return 1;
  }
  for (int th = 0; th <= 5; ++th)
    if (!g_th[th]) {
      fprintf(stderr, "t >> 32 == %d never reached\n", th);
      return 1;
    }
  const uint64_t ub = g_ubranch, wb = g_wbranch;
  // Random values: any wrap count a sum of up to 300 terms reaches, and any hi at all.
  std::mt19937_64 rng(20261020);
  for (int i = 0; i < 10000000; ++i) {
    const uint64_t lo = rng(), r = rng();
    const uint32_t hi = (i & 1) ? (uint32_t)(r % 301) : (uint32_t)r;
    if (!check(((u128)hi << 64) | lo)) return 1;
  }
  printf("fold96: %llu built and matrix-core-range values (u >> 32 == 1 taken %llu times, w >= p %llu times) and 10000000 random bit-exact\n",
         (unsigned long long)(g_n - 10000000), (unsigned long long)ub, (unsigned long long)wb);
  return 0;
}
