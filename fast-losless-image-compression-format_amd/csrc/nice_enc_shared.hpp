// nice_enc_shared.hpp -- what more than one of the encoder's files
// (nice_classify.hip, nice_pack.hip, nice_encode.hip) use: the "no pixel"
// value, the tile mask scan, the mode prefixes' identifying streams, the
// work-item iterator and the wrapped write.  Device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nice_format.h"
#include "nice_kernels.h"
#include "nice_pack.hpp"

namespace nice {

constexpr uint32_t NONE = 0xFFFFFFFFu;

// Next coded pixel strictly after local index p, using the tile's coded bitmask
// (ENC_TILE bits). Returns ENC_TILE if none inside the tile.
__device__ __forceinline__ int next_coded_local(const uint32_t* mask, int p) {
  int w = (p + 1) >> 5;
  const int b = (p + 1) & 31;
  if (p + 1 >= ENC_TILE) return ENC_TILE;
  uint32_t m = mask[w] & (b ? (0xFFFFFFFFu << b) : 0xFFFFFFFFu);
  while (true) {
    if (m) return (w << 5) + __builtin_ctz(m);
    ++w;
    if (w >= ENC_TILE / 32) return ENC_TILE;
    m = mask[w];
  }
}

// Each mode's identifying stream and symbols per pixel (code.rs:191-366):
// BACK_REF one SC_BACK_REF symbol, RGB three SC_RGB, LUMA one
// SC_LUMA_BACK_REF, SMALL_DIFF one SC_SMALL_DIFF1, LUMA2 one
// SC_LUMA_BASE_DIFF2 -- so a mode's prefix count is its stream's total
// divided by that number, and the classify pass does not count prefixes.
__device__ __forceinline__ bool mode_id_bin(int k, int b) {
  const int lo = k == P_BACK_REF ? BIN_BACK_REF : k == P_RGB ? 0 : k == P_LUMA ? BIN_LUMA_REF
               : k == P_SMALL_DIFF ? BIN_SMALL_DIFF : BIN_LUMA2_BASE;
  const int n = k == P_BACK_REF ? N_BINS - BIN_BACK_REF : k == P_RGB ? 256 : k == P_LUMA ? 11
              : k == P_SMALL_DIFF ? 343 : 64;
  return b >= lo && b < lo + n;
}
__device__ __forceinline__ uint32_t mode_id_syms(int k) { return k == P_RGB ? 3u : 1u; }

// Work item -> (frame, tile) without a 64-bit division per tile (one at the
// start; the scalar division sequence is ~100 instructions).
struct TileIter {
  uint32_t f, k, nt, lo, T;
  __device__ __forceinline__ TileIter(const EncArgs& a, uint64_t w)
      : f((uint32_t)(w / (a.tile_hi - a.tile_lo))), k((uint32_t)(w % (a.tile_hi - a.tile_lo))),
        nt(a.tile_hi - a.tile_lo), lo(a.tile_lo), T(a.tiles_per_frame) {}
  __device__ __forceinline__ void step(uint32_t n) {
    k += n;
    while (k >= nt) { k -= nt; ++f; }
  }
  __device__ __forceinline__ uint32_t tt() const { return lo + k; }
  __device__ __forceinline__ uint64_t tile() const { return (uint64_t)f * T + lo + k; }
};

// A write the reference's u32 cache wraps (nice_pack.hpp pack_wrapped_window;
// nice_pack.hip "Long codes"): the 32-bit window at the byte of stream bit p,
// read and written back byte by byte (enc_pack_long phase 1, enc_band_fix).
__device__ __forceinline__ void wrapped_write(uint8_t* out, uint64_t p, uint32_t v, uint32_t n) {
  const uint64_t B = p >> 3;
  const uint32_t w = ((uint32_t)out[B] << 24) | ((uint32_t)out[B + 1] << 16) | ((uint32_t)out[B + 2] << 8) | out[B + 3];
  const uint32_t r = pack_wrapped_window(w, (uint32_t)(p & 7u), v, n);
  out[B] = (uint8_t)(r >> 24);
  out[B + 1] = (uint8_t)(r >> 16);
  out[B + 2] = (uint8_t)(r >> 8);
  out[B + 3] = (uint8_t)r;
}

}  // namespace nice
