// nice_tile_geom.hpp -- the geometry every tile-to-window kernel shares
// (nice_tiles.hip, nice_sets.hip, nice_sets_tensor.hip, nice_sets_resize.hip):
// the cut of a tile to its band, window and image, the split of a wave between
// the groups of a row and the rows below it, and the widest vector a base and
// its pitches allow.  No HIP: a plain C++ compiler reads it too
// (tools/tile_geom_check.cpp, tests/test_tile_geom_arith.py).
#pragma once
#include <stdint.h>

#include "nice_geom.h"

namespace nice {

// Pixels [xa, xa + nxp) x [ya, yb) of the image; the tile's origin is (tx0, ty0).
struct TileCut {
  uint32_t xa, nxp, ya, yb, tx0, ty0;
  bool empty;   // nothing to move: the other fields are not to be used
};

// Tile t (row-major in a grid nx tiles wide) of tw x th pixels, its band
// `band` of rows_pb rows, cut to the rectangle (x0, y0, rw, rh) and to the
// w x h image.  64-bit throughout: x0 + rw, a tile's far edge and a band's end
// may pass 2^32 where the result does not.
NICE_HDI TileCut tile_cut(uint32_t t, uint32_t nx, uint32_t tw, uint32_t th, uint32_t band, uint32_t rows_pb, uint32_t x0,
                          uint32_t y0, uint32_t rw, uint32_t rh, uint32_t w, uint32_t h) {
  const auto lo = [](uint64_t a, uint64_t b) { return a < b ? a : b; };
  const auto hi = [](uint64_t a, uint64_t b) { return a > b ? a : b; };
  const uint32_t ty = t / nx, tx = t % nx;
  const uint64_t tx0 = (uint64_t)tx * tw, ty0 = (uint64_t)ty * th;
  const uint64_t xa64 = hi(tx0, (uint64_t)x0);
  const uint64_t xb64 = lo(lo(tx0 + tw, (uint64_t)x0 + rw), (uint64_t)w);
  const uint64_t ya64 = hi(ty0 + (uint64_t)band * rows_pb, (uint64_t)y0);
  const uint64_t yb64 = lo(lo(ty0 + lo((uint64_t)(band + 1) * rows_pb, (uint64_t)th), (uint64_t)y0 + rh), (uint64_t)h);
  const bool empty = xa64 >= xb64 || ya64 >= yb64;
  return TileCut{(uint32_t)xa64, (uint32_t)(xb64 - xa64), (uint32_t)ya64, (uint32_t)yb64, (uint32_t)tx0, (uint32_t)ty0, empty};
}

// A row of `groups` lane-sized groups: lpr = 1 << ls lanes per row, the power
// of two that holds the groups, up to the wave; the wave's other lanes take
// the rpw - 1 rows below (lpr * rpw == 64).
struct RowShare {
  uint32_t ls, lpr, rpw;
};
NICE_HDI RowShare row_share(uint32_t groups) {
  uint32_t ls = 0;
  while (ls < 6u && (1u << ls) < groups) ++ls;
  return RowShare{ls, 1u << ls, 64u >> ls};
}

// The widest mode lp <= max_lp such that a lane's 1 << lp consecutive elements
// of elem_bytes bytes are one aligned vector in every row and plane: the base
// is aligned to the vector, and the pitches (in elements; plane_pitch 0: no
// planes) and `edge`, the column the lanes' groups count from, are multiples of
// its elements.
NICE_HDI uint32_t vector_mode(uint64_t base, uint64_t elem_bytes, uint64_t row_pitch, uint64_t plane_pitch, uint64_t edge,
                              uint32_t max_lp) {
  uint32_t mode = 0;
  for (uint32_t lp = 1; lp <= max_lp; ++lp) {
    const uint64_t p = 1ull << lp;
    if ((base & (p * elem_bytes - 1)) || ((row_pitch | plane_pitch | edge) & (p - 1))) break;
    mode = lp;
  }
  return mode;
}

// vector_mode for the byte-moving kernels, whose pixels are 4 bytes and whose
// modes are 0: bytes, 1: one pixel as a dword, 2: four pixels as 16 bytes
// (TileMode, nice_tiles.hpp): base and pitch in bytes, x0 the pixel column the
// groups count from.
NICE_HDI uint32_t byte_mode(uint64_t base, uint64_t pitch, uint64_t x0) {
  const uint32_t lp = vector_mode(base, 1, pitch, 0, 4 * x0, 4);
  return lp == 4 ? 2u : lp >= 2 ? 1u : 0u;
}

}  // namespace nice
