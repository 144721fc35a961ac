// nice_tiles.hpp -- what the byte-moving kernels of nice_tiles.hip (one tiled
// image) and nice_sets.hip (image sets) share: the block and unroll constants,
// the three move modes, the pixel loads and stores, and the band geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace nice {

constexpr uint32_t TL_THREADS = 256;
constexpr uint32_t TL_WAVES = TL_THREADS / 64;
constexpr uint32_t TL_UNROLL = 4;            // 4 x 1 KiB of loads in flight per wave on the 16-byte path
constexpr uint32_t TL_BLOCK_BYTES = 32768;   // a block's band of tile rows: about this many bytes

// how a row is moved: per pixel byte by byte (any channels, any alignment),
// per RGBA pixel as one dword, or four RGBA pixels as 16 bytes
enum TileMode { TL_BYTES = 0, TL_DWORD = 1, TL_QUAD = 2 };

__device__ __forceinline__ uint32_t tl_wave() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }

// One pixel of `c` (3 or 4) bytes at p, byte loads: bytes +0..+2 in the low 24
// bits, byte +3 (c == 4) or `fill` on top.
__device__ __forceinline__ uint32_t ld_px_bytes(const uint8_t* p, uint32_t c, uint32_t fill) {
  const uint32_t b0 = p[0], b1 = p[1], b2 = p[2];
  const uint32_t b3 = c == 4 ? (uint32_t)p[3] : fill;
  return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}
__device__ __forceinline__ void st_px_bytes(uint8_t* p, uint32_t c, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
  p[2] = (uint8_t)(v >> 16);
  if (c == 4) p[3] = (uint8_t)(v >> 24);
}

// Blocks per tile and tile rows per block for rows of row_bytes; false if
// slots * bands blocks do not fit a launch grid.
inline bool tl_bands(uint32_t slots, uint32_t th, uint64_t row_bytes, uint32_t& bands, uint32_t& rows_pb) {
  uint64_t rows = TL_BLOCK_BYTES / std::max<uint64_t>(row_bytes, 1);
  rows = std::min<uint64_t>(std::max<uint64_t>(rows, TL_WAVES), th);
  rows_pb = (uint32_t)rows;
  bands = (th + rows_pb - 1) / rows_pb;
  return (uint64_t)slots * bands <= 0x7FFFFFFFull;
}
inline bool tl_aligned(const void* p, uint64_t s, uint32_t a) { return ((uintptr_t)p & (a - 1)) == 0 && (s & (a - 1)) == 0; }

// ---- the alpha kernels' rows (one image: nice_tiles.hip; a set: nice_sets.hip) ----
// One wave, one row; everything but `lane` is wave-uniform.

// mn / mx take byte +3 of pixels [xs, xe) of the image row at srow (w pixels, xe <= w).
template <int MODE>
__device__ __forceinline__ void alpha_range_row(const uint8_t* srow, uint32_t w, uint32_t xs, uint32_t xe, uint32_t lane,
                                                uint32_t& mn, uint32_t& mx) {
  const uint32_t xl = w - 1;
  if (MODE == TL_QUAD) {   // the 16-byte groups of the row that hold [xs, xe)
    const uint32_t gb = xs >> 2, ge = (xe + 3u) >> 2;
    for (uint32_t g0 = gb; g0 < ge; g0 += 64u * TL_UNROLL) {
      uint4 v[TL_UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < TL_UNROLL; ++u) {
        const uint32_t g = g0 + 64u * u + lane;
        if (g < ge) {
          const uint32_t x = 4u * g;
          if (x + 4u <= w) {
            v[u] = *reinterpret_cast<const uint4*>(srow + 16ull * g);
          } else {   // the image ends inside this group
            v[u].x = ld32(srow + 4ull * x);
            v[u].y = ld32(srow + 4ull * min(x + 1u, xl));
            v[u].z = ld32(srow + 4ull * min(x + 2u, xl));
            v[u].w = ld32(srow + 4ull * min(x + 3u, xl));
          }
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < TL_UNROLL; ++u) {
        const uint32_t g = g0 + 64u * u + lane;
        if (g < ge) {
          const uint32_t x = 4u * g;
          const uint32_t a[4] = {v[u].x >> 24, v[u].y >> 24, v[u].z >> 24, v[u].w >> 24};
#pragma unroll
          for (uint32_t k = 0; k < 4; ++k) {
            if (x + k >= xs && x + k < xe) {   // the tile's own pixels of the group
              mn = min(mn, a[k]);
              mx = max(mx, a[k]);
            }
          }
        }
      }
    }
  } else {
    const uint32_t nxp = xe - xs;
    for (uint32_t g0 = 0; g0 < nxp; g0 += 64u * TL_UNROLL) {
      uint32_t a[TL_UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < TL_UNROLL; ++u) {
        const uint32_t g = g0 + 64u * u + lane;
        if (g < nxp) {
          const uint8_t* s = srow + 4ull * (xs + g);
          a[u] = MODE == TL_DWORD ? ld32(s) >> 24 : (uint32_t)s[3];
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < TL_UNROLL; ++u) {
        const uint32_t g = g0 + 64u * u + lane;
        if (g < nxp) {
          mn = min(mn, a[u]);
          mx = max(mx, a[u]);
        }
      }
    }
  }
}

// The wave's mn / mx into *lo / *hi (preset to 255 / 0); a wave without rows has nothing to say.
__device__ __forceinline__ void alpha_range_commit(uint32_t mn, uint32_t mx, uint32_t lane, uint32_t* lo, uint32_t* hi) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, d, 64));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
  }
  if (lane == 0 && mn <= mx) {
    atomicMin(lo, mn);
    atomicMax(hi, mx);
  }
}

// Triplet row: drow[j], j < aw3, takes byte +3 of the image row's pixel at the
// twice clamped column (to the tile's last, xs + tw - 1, then to the image's, xl).
__device__ __forceinline__ void alpha_gather_row(const uint8_t* srow, uint8_t* drow, uint32_t aw3, uint32_t xs, uint32_t tw,
                                                 uint32_t xl, uint32_t lane) {
  for (uint32_t g0 = 0; g0 < aw3; g0 += 64u * TL_UNROLL) {
    uint8_t v[TL_UNROLL];
#pragma unroll
    for (uint32_t u = 0; u < TL_UNROLL; ++u) {
      const uint32_t g = g0 + 64u * u + lane;
      if (g < aw3) v[u] = srow[4ull * min(xs + min(g, tw - 1u), xl) + 3u];
    }
#pragma unroll
    for (uint32_t u = 0; u < TL_UNROLL; ++u) {
      const uint32_t g = g0 + 64u * u + lane;
      if (g < aw3) drow[g] = v[u];
    }
  }
}

// Byte +3 of the nxp 4-byte pixels at drow from the plane row at srow, or from
// the constant cval (cst).  TL_QUAD: drow is 16-byte aligned, and a lane
// rewrites four pixels' alpha as one 16-byte read-modify-write (the colour
// bytes come back as they were); the group the row ends in, and every other
// mode, stores bytes.
template <int MODE>
__device__ __forceinline__ void alpha_merge_row(const uint8_t* srow, uint8_t* drow, uint32_t nxp, bool cst, uint32_t cval,
                                                uint32_t lane) {
  if (MODE == TL_QUAD) {
    const uint32_t G = (nxp + 3u) >> 2;
    for (uint32_t g0 = 0; g0 < G; g0 += 64u * TL_UNROLL) {
      uint4 v[TL_UNROLL];
      uint32_t al4[TL_UNROLL];   // four alpha bytes, pixel k in bits 8k..8k+7
#pragma unroll
      for (uint32_t u = 0; u < TL_UNROLL; ++u) {
        const uint32_t g = g0 + 64u * u + lane;
        if (g < G) {
          const uint32_t k = min(nxp - 4u * g, 4u);   // pixels of the group: 1..4
          if (k == 4u) v[u] = *reinterpret_cast<const uint4*>(drow + 16ull * g);
          uint32_t p = cval * 0x01010101u;
          if (!cst) {
            const uint8_t* s = srow + 4u * g;
            p = s[0];
            if (k > 1) p |= (uint32_t)s[1] << 8;
            if (k > 2) p |= (uint32_t)s[2] << 16;
            if (k > 3) p |= (uint32_t)s[3] << 24;
          }
          al4[u] = p;
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < TL_UNROLL; ++u) {
        const uint32_t g = g0 + 64u * u + lane;
        if (g < G) {
          uint8_t* d = drow + 16ull * g;
          const uint32_t k = min(nxp - 4u * g, 4u), p = al4[u];
          if (k == 4u) {
            v[u].x = (v[u].x & 0xFFFFFFu) | (p << 24);
            v[u].y = (v[u].y & 0xFFFFFFu) | ((p >> 8) << 24);
            v[u].z = (v[u].z & 0xFFFFFFu) | ((p >> 16) << 24);
            v[u].w = (v[u].w & 0xFFFFFFu) | ((p >> 24) << 24);
            *reinterpret_cast<uint4*>(d) = v[u];
          } else {
            d[3] = (uint8_t)p;
            if (k > 1) d[7] = (uint8_t)(p >> 8);
            if (k > 2) d[11] = (uint8_t)(p >> 16);
          }
        }
      }
    }
  } else {
    for (uint32_t g0 = 0; g0 < nxp; g0 += 64u * TL_UNROLL) {
      uint8_t v[TL_UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < TL_UNROLL; ++u) {
        const uint32_t g = g0 + 64u * u + lane;
        if (g < nxp) v[u] = cst ? (uint8_t)cval : srow[g];
      }
#pragma unroll
      for (uint32_t u = 0; u < TL_UNROLL; ++u) {
        const uint32_t g = g0 + 64u * u + lane;
        if (g < nxp) drow[4ull * g + 3u] = v[u];
      }
    }
  }
}

}  // namespace nice
