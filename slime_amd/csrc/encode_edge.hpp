// Edge geometry of one object of a ragged byte encode (rs_bytes_ragged_encode.hip).
// Pure arithmetic, host and device: tests/cpp/encode_edge_test.cpp builds it with
// plain g++.
//
// An object of S bytes is cut into k data chunks of L columns (4-byte words),
// chunk j holding object words [jL, (j+1)L).  Word w < nw = ceil(S/4) carries
// object bytes (the last one partially when S % 4 != 0); words nw .. kL-1 are
// splitVector's padding.  nw is clamped to kL, so a size that contradicts L can
// never name a word outside the object's own chunks.
//
// Column c of the chunks is INTERIOR when word jL + c is a whole object word in
// every data chunk j -- the last chunk decides.  Vectors (4 columns) below
// `interior` are interior in all four columns: the walk encodes them without a
// check.  The columns from 4 * interior to L - 1 are the object's EDGE columns;
// with L = ceil(nw / k) (slime_rs_chunk_size) there are at most
// edge_columns_max(k) = k + 3 of them: at most k - 1 padding words, the partial
// word, and three columns of rounding down to a whole vector.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SLIME_EDGE_HD __host__ __device__
#else
#define SLIME_EDGE_HD
#endif

namespace slime {
namespace edge {

struct Geom {
  uint64_t nw;        // words carrying object bytes, clamped to kL
  uint32_t tailmask;  // valid high bytes of word nw-1 (0xFFFFFFFF when it is whole)
  uint32_t interior;  // interior 16-byte vectors, at most L / 4
};

SLIME_EDGE_HD inline Geom geom(uint64_t S, uint64_t L, uint32_t k) {
  const uint64_t cap = (uint64_t)k * L, full = S / 4 + (S % 4 ? 1 : 0);
  Geom g;
  g.nw = full < cap ? full : cap;
  const bool partial = S % 4 != 0 && g.nw == full;
  g.tailmask = partial ? 0xFFFFFFFFu << (8 * (4 - S % 4)) : 0xFFFFFFFFu;
  const uint64_t whole = partial ? g.nw - 1 : g.nw;
  const uint64_t lim = (uint64_t)(k - 1) * L;  // first word of the last data chunk
  g.interior = whole > lim ? (uint32_t)((whole - lim) / 4) : 0u;  // whole - lim <= L < 2^30
  return g;
}

// Edge columns of an object whose L is slime_rs_chunk_size(S, k) / 4.
SLIME_EDGE_HD inline uint32_t edge_columns_max(uint32_t k) { return k + 3; }

}  // namespace edge
}  // namespace slime
