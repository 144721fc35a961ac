// nice_tiles.hip -- tiled images (include/nice.h, "Tiled images"): the copies
// between one pitched image and its dense, equally sized tiles, the compare
// behind the encoder's verify pass, the raw fallback of a tile the format
// cannot carry, and the alpha batch's kernels (per-tile range, triplet gather,
// verdict and raw store, pack, merge).  All of it moves bytes: a block takes a
// band of rows of one tile, a wave one row at a time, a lane one pixel (or
// four, 16 bytes; the alpha kernels one byte, or the alpha of four pixels).
// Everything but the lane's column is wave-uniform; a lane's loads are issued
// before its stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/nice.h"
#include "nice_internal.h"
#include "nice_tile_geom.hpp"
#include "nice_tiles.hpp"

namespace nice {

struct TileGrid {
  uint32_t w, h, tw, th, nx;
  uint32_t bands, rows_pb;   // blocks per tile, tile rows per block
};

// Image -> tiles.  Tile position (r, g) takes the image pixel at the clamped
// coordinate (min(x, w - 1), min(y, h - 1)): every load is inside the image,
// every store inside the tile.
template <int MODE>
__global__ __launch_bounds__(TL_THREADS) void tiles_split(const uint8_t* __restrict__ img, uint64_t pitch, uint32_t C,
                                                          TileGrid q, uint8_t* __restrict__ tiles,
                                                          uint64_t tile_stride) {
  const uint32_t t = blockIdx.x / q.bands, band = blockIdx.x % q.bands;
  const uint32_t ty = t / q.nx, tx = t % q.nx;
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  const uint32_t r0 = band * q.rows_pb, r1 = min(r0 + q.rows_pb, q.th);
  const uint32_t x0 = tx * q.tw, xl = q.w - 1;
  uint8_t* dt = tiles + (uint64_t)t * tile_stride;
  for (uint32_t r = r0 + wave; r < r1; r += TL_WAVES) {
    const uint32_t y = min(ty * q.th + r, q.h - 1);
    const uint8_t* srow = img + (uint64_t)y * pitch;
    uint8_t* drow = dt + (uint64_t)r * q.tw * C;
    if (MODE == TL_QUAD) {
      const uint32_t G = q.tw >> 2;
      for (uint32_t g0 = 0; g0 < G; g0 += 64u * TL_UNROLL) {
        uint4 v[TL_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) {
          const uint32_t g = g0 + 64u * u + lane;
          if (g < G) {
            const uint32_t x = x0 + 4u * g;
            if (x + 4u <= q.w) {
              v[u] = *reinterpret_cast<const uint4*>(srow + 4ull * x);
            } else {   // the image's right edge runs through or before this group
              v[u].x = ld32(srow + 4ull * min(x, xl));
              v[u].y = ld32(srow + 4ull * min(x + 1u, xl));
              v[u].z = ld32(srow + 4ull * min(x + 2u, xl));
              v[u].w = ld32(srow + 4ull * min(x + 3u, xl));
            }
          }
        }
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) {
          const uint32_t g = g0 + 64u * u + lane;
          if (g < G) *reinterpret_cast<uint4*>(drow + 16ull * g) = v[u];
        }
      }
    } else {
      for (uint32_t g0 = 0; g0 < q.tw; g0 += 64u * TL_UNROLL) {
        uint32_t v[TL_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) {
          const uint32_t g = g0 + 64u * u + lane;
          if (g < q.tw) {
            const uint8_t* s = srow + (uint64_t)min(x0 + g, xl) * C;
            v[u] = MODE == TL_DWORD ? ld32(s) : ld_px_bytes(s, C, 0u);
          }
        }
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) {
          const uint32_t g = g0 + 64u * u + lane;
          if (g < q.tw) {
            if (MODE == TL_DWORD) *reinterpret_cast<uint32_t*>(drow + 4ull * g) = v[u];
            else st_px_bytes(drow + (uint64_t)g * C, C, v[u]);
          }
        }
      }
    }
  }
}

struct MergeArgs {
  const uint8_t* tiles;
  uint64_t tile_stride;
  const unsigned long long* src_off;   // non-null: slot i at tiles + src_off[i]
  const uint32_t* tile_idx;
  const int32_t* slot_status;          // non-null: a slot with a nonzero status is skipped
  uint32_t n_tiles;                    // nx * ny
  uint32_t x0, y0, rw, rh;
  uint32_t tc, oc, fill;               // bytes per pixel in the slots, in the window; byte +3 when tc == 3
  uint8_t* out;
  uint64_t out_pitch;
};

// Tiles -> window.  Slot i's tile, cut to the rectangle and to the image (no
// padding is ever written), goes to out + (y - y0) * out_pitch + (x - x0) * oc.
template <int MODE>
__global__ __launch_bounds__(TL_THREADS) void tiles_merge(MergeArgs a, TileGrid q) {
  const uint32_t slot = blockIdx.x / q.bands, band = blockIdx.x % q.bands;
  if (a.slot_status && a.slot_status[slot] != 0) return;
  const uint32_t t = a.tile_idx[slot];
  if (t >= a.n_tiles) return;
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  // the tile's pixels inside the rectangle and the image
  const TileCut c = tile_cut(t, q.nx, q.tw, q.th, band, q.rows_pb, a.x0, a.y0, a.rw, a.rh, q.w, q.h);
  if (c.empty) return;
  const uint32_t xa = c.xa, nxp = c.nxp, ya = c.ya, yb = c.yb;
  const uint8_t* st = a.tiles + (a.src_off ? (uint64_t)a.src_off[slot] : (uint64_t)slot * a.tile_stride);
  for (uint32_t y = ya + wave; y < yb; y += TL_WAVES) {
    const uint8_t* srow = st + ((uint64_t)(y - c.ty0) * q.tw + (xa - c.tx0)) * a.tc;
    uint8_t* drow = a.out + (uint64_t)(y - a.y0) * a.out_pitch + (uint64_t)(xa - a.x0) * a.oc;
    if (MODE == TL_QUAD) {   // xa, x0 and the tile's x origin are multiples of 4: both rows are 16-byte aligned
      const uint32_t G = (nxp + 3u) >> 2;
      for (uint32_t g0 = 0; g0 < G; g0 += 64u * TL_UNROLL) {
        uint4 v[TL_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) {
          const uint32_t g = g0 + 64u * u + lane;
          // (the source group is whole inside the tile: tw % 4 == 0)
          if (g < G) v[u] = *reinterpret_cast<const uint4*>(srow + 16ull * g);
        }
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) {
          const uint32_t g = g0 + 64u * u + lane;
          if (g < G) {
            uint8_t* d = drow + 16ull * g;
            if (4u * g + 4u <= nxp) {
              *reinterpret_cast<uint4*>(d) = v[u];
            } else {   // the window or the image ends inside this group
              const uint32_t k = nxp - 4u * g;   // 1..3 pixels
              *reinterpret_cast<uint32_t*>(d) = v[u].x;
              if (k > 1) *reinterpret_cast<uint32_t*>(d + 4) = v[u].y;
              if (k > 2) *reinterpret_cast<uint32_t*>(d + 8) = v[u].z;
            }
          }
        }
      }
    } else {
      for (uint32_t g0 = 0; g0 < nxp; g0 += 64u * TL_UNROLL) {
        uint32_t v[TL_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) {
          const uint32_t g = g0 + 64u * u + lane;
          if (g < nxp) v[u] = MODE == TL_DWORD ? ld32(srow + 4ull * g) : ld_px_bytes(srow + (uint64_t)g * a.tc, a.tc, a.fill);
        }
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) {
          const uint32_t g = g0 + 64u * u + lane;
          if (g < nxp) {
            if (MODE == TL_DWORD) *reinterpret_cast<uint32_t*>(drow + 4ull * g) = v[u];
            else st_px_bytes(drow + (uint64_t)g * a.oc, a.oc, v[u]);
          }
        }
      }
    }
  }
}

// kind[t] = 1 where bytes +0..+2 of some pixel of tile t differ between the two
// arrays or status[t] != 0 (kind is zeroed before the launch; every writer
// stores the same 1).  dword: both arrays hold 4-byte aligned RGBA pixels.
__global__ __launch_bounds__(TL_THREADS) void tiles_compare(const uint8_t* __restrict__ A, uint64_t stride_a,
                                                            const uint8_t* __restrict__ B, uint64_t stride_b,
                                                            uint32_t C, uint32_t npx, uint32_t chunks, uint32_t per,
                                                            int dword, const int32_t* __restrict__ status,
                                                            uint8_t* __restrict__ kind) {
  const uint32_t t = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  if (status[t] != 0) {   // nothing to compare: the decode wrote no defined pixels
    if (chunk == 0 && threadIdx.x == 0) kind[t] = 1;
    return;
  }
  const uint8_t* a = A + (uint64_t)t * stride_a;
  const uint8_t* b = B + (uint64_t)t * stride_b;
  const uint64_t p0 = (uint64_t)chunk * per;
  const uint32_t p1 = (uint32_t)min(p0 + per, (uint64_t)npx);
  bool diff = false;
  for (uint64_t pb = p0; pb < p1; pb += (uint64_t)TL_THREADS * TL_UNROLL) {
    uint32_t va[TL_UNROLL], vb[TL_UNROLL];
#pragma unroll
    for (uint32_t u = 0; u < TL_UNROLL; ++u) {
      const uint64_t p = pb + (uint64_t)u * TL_THREADS + threadIdx.x;
      va[u] = vb[u] = 0;
      if (p < p1) {
        va[u] = dword ? ld32(a + 4ull * p) : ld_px_bytes(a + p * C, 3, 0u);
        vb[u] = dword ? ld32(b + 4ull * p) : ld_px_bytes(b + p * C, 3, 0u);
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < TL_UNROLL; ++u) diff |= ((va[u] ^ vb[u]) & 0xFFFFFFu) != 0;
  }
  if (__ballot(diff) != 0ull && (threadIdx.x & 63u) == 0) kind[t] = 1;
}

// A tile with kind[t] == 1: its slot takes the tile's RGB (3 bytes per pixel,
// row-major) and len[t] their count.
__global__ __launch_bounds__(TL_THREADS) void tiles_store_raw(const uint8_t* __restrict__ tiles, uint64_t tile_stride,
                                                              uint32_t C, uint32_t npx, uint32_t chunks, uint32_t per,
                                                              const uint8_t* __restrict__ kind,
                                                              uint8_t* __restrict__ slots, uint64_t slot_stride,
                                                              unsigned long long* __restrict__ len) {
  const uint32_t t = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  if (kind[t] == 0) return;
  if (chunk == 0 && threadIdx.x == 0) len[t] = 3ull * npx;
  const uint8_t* s = tiles + (uint64_t)t * tile_stride;
  uint8_t* d = slots + (uint64_t)t * slot_stride;
  const uint64_t p0 = (uint64_t)chunk * per;
  const uint32_t p1 = (uint32_t)min(p0 + per, (uint64_t)npx);
  for (uint64_t pb = p0; pb < p1; pb += (uint64_t)TL_THREADS * TL_UNROLL) {
    uint32_t v[TL_UNROLL];
#pragma unroll
    for (uint32_t u = 0; u < TL_UNROLL; ++u) {
      const uint64_t p = pb + (uint64_t)u * TL_THREADS + threadIdx.x;
      if (p < p1) v[u] = ld_px_bytes(s + p * C, 3, 0u);
    }
#pragma unroll
    for (uint32_t u = 0; u < TL_UNROLL; ++u) {
      const uint64_t p = pb + (uint64_t)u * TL_THREADS + threadIdx.x;
      if (p < p1) st_px_bytes(d + 3ull * p, 3, v[u]);
    }
  }
}

// out[pos[i]] = st[i]: the coded tiles' decode statuses to their places among the selected tiles
__global__ void tiles_scatter_status(const int32_t* __restrict__ st, const uint32_t* __restrict__ pos, uint32_t n,
                                     int32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[pos[i]] = st[i];
}

// ---- alpha (include/nice.h, "tiled images", alpha) ---------------------------
// Byte +3 of an RGBA image, tile by tile.  The alpha plane of a tile is coded
// as its triplet image: aw = ceil(tile_w / 3) pixels of 3 bytes per row, so a
// triplet row is the plane's row with its last byte repeated up to 3 * aw.

// lo[t] / hi[t] = min / max of byte +3 over tile t (preset to 255 / 0).  Only
// pixels inside the image are read: the padding repeats pixels of the same tile.
template <int MODE>
__global__ __launch_bounds__(TL_THREADS) void alpha_range(const uint8_t* __restrict__ img, uint64_t pitch, TileGrid q,
                                                          uint32_t* __restrict__ lo, uint32_t* __restrict__ hi) {
  const uint32_t t = blockIdx.x / q.bands, band = blockIdx.x % q.bands;
  const uint32_t ty = t / q.nx, tx = t % q.nx;
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  const uint32_t xs = tx * q.tw, xe = min(xs + q.tw, q.w);
  const uint32_t ys = ty * q.th + band * q.rows_pb;
  const uint32_t ye = min(ty * q.th + min((band + 1) * q.rows_pb, q.th), q.h);
  uint32_t mn = 255u, mx = 0u;
  for (uint32_t y = ys + wave; y < ye; y += TL_WAVES)
    alpha_range_row<MODE>(img + (uint64_t)y * pitch, q.w, xs, xe, lane, mn, mx);
  alpha_range_commit(mn, mx, lane, &lo[t], &hi[t]);
}

// Triplet image of tile list[i] at trip + i * trip_stride: byte j of row r is
// byte +3 of the pixel at the twice clamped coordinate (to the tile's last
// column, then to the image).
__global__ __launch_bounds__(TL_THREADS) void alpha_gather(const uint8_t* __restrict__ img, uint64_t pitch, TileGrid q,
                                                           const uint32_t* __restrict__ list, uint32_t aw3,
                                                           uint8_t* __restrict__ trip, uint64_t trip_stride) {
  const uint32_t i = blockIdx.x / q.bands, band = blockIdx.x % q.bands;
  const uint32_t t = list[i];
  const uint32_t ty = t / q.nx, tx = t % q.nx;
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  const uint32_t r0 = band * q.rows_pb, r1 = min(r0 + q.rows_pb, q.th);
  const uint32_t xs = tx * q.tw, xl = q.w - 1;
  uint8_t* dt = trip + (uint64_t)i * trip_stride;
  for (uint32_t r = r0 + wave; r < r1; r += TL_WAVES) {
    const uint8_t* srow = img + (uint64_t)min(ty * q.th + r, q.h - 1) * pitch;
    alpha_gather_row(srow, dt + (uint64_t)r * aw3, aw3, xs, q.tw, xl, lane);
  }
}

// The verdict of stream i (tile list[i]): raw (1) where the verify compare set
// vk[i] or the stream is not shorter than the plane's npx bytes.  The tile's
// entries of the n-entry tables are written, mlen[i] becomes the stored length
// and the slot's bytes from there to the next multiple of 16 are zeroed.
__global__ void alpha_verdict(const uint32_t* __restrict__ list, uint32_t m, uint32_t npx, uint8_t* __restrict__ vk,
                              unsigned long long* __restrict__ mlen, uint8_t* __restrict__ slots, uint64_t slot_stride,
                              uint8_t* __restrict__ akind, unsigned long long* __restrict__ alen) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t raw = (vk[i] != 0 || mlen[i] >= npx) ? 1u : 0u;
  const unsigned long long l = raw ? (unsigned long long)npx : mlen[i];
  vk[i] = (uint8_t)raw;
  mlen[i] = l;
  akind[list[i]] = (uint8_t)raw;
  alen[list[i]] = l;
  uint8_t* s = slots + (uint64_t)i * slot_stride;
  for (unsigned long long b = l; (b & 15ull) != 0; ++b) s[b] = 0;
}

// A stream with vk[i] == 1: its slot takes the plane, tw bytes per row (the
// first tw bytes of the triplet row).
__global__ __launch_bounds__(TL_THREADS) void alpha_store_raw(const uint8_t* __restrict__ trip, uint64_t trip_stride,
                                                              uint32_t aw3, TileGrid q, const uint8_t* __restrict__ vk,
                                                              uint8_t* __restrict__ slots, uint64_t slot_stride) {
  const uint32_t i = blockIdx.x / q.bands, band = blockIdx.x % q.bands;
  if (vk[i] == 0) return;
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  const uint32_t r0 = band * q.rows_pb, r1 = min(r0 + q.rows_pb, q.th);
  for (uint32_t r = r0 + wave; r < r1; r += TL_WAVES) {
    const uint8_t* srow = trip + (uint64_t)i * trip_stride + (uint64_t)r * aw3;
    uint8_t* drow = slots + (uint64_t)i * slot_stride + (uint64_t)r * q.tw;
    for (uint32_t g0 = 0; g0 < q.tw; g0 += 64u * TL_UNROLL) {
      uint8_t v[TL_UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < TL_UNROLL; ++u) {
        const uint32_t g = g0 + 64u * u + lane;
        if (g < q.tw) v[u] = srow[g];
      }
#pragma unroll
      for (uint32_t u = 0; u < TL_UNROLL; ++u) {
        const uint32_t g = g0 + 64u * u + lane;
        if (g < q.tw) drow[g] = v[u];
      }
    }
  }
}

// Slot i (16-byte aligned, pad bytes already zero) -> packed + off[list[i]],
// whole 16-byte granules; no granule that would end past cap is written.
constexpr uint32_t AL_PACK_GRANULES = TL_THREADS * TL_UNROLL * 4;   // per block: 64 KiB
__global__ __launch_bounds__(TL_THREADS) void alpha_pack(const uint8_t* __restrict__ slots, uint64_t slot_stride,
                                                         const unsigned long long* __restrict__ mlen,
                                                         const uint32_t* __restrict__ list, uint32_t chunks,
                                                         const unsigned long long* __restrict__ off,
                                                         uint8_t* __restrict__ packed, unsigned long long cap) {
  const uint32_t i = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const unsigned long long G = (mlen[i] + 15ull) >> 4;
  const unsigned long long d0 = off[list[i]] >> 4;
  const unsigned long long Gw = cap >> 4 > d0 ? min(G, (cap >> 4) - d0) : 0ull;   // granules that may be written
  const unsigned long long k0 = (unsigned long long)chunk * AL_PACK_GRANULES;
  const unsigned long long k1 = min(k0 + AL_PACK_GRANULES, Gw);
  const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(slots + (uint64_t)i * slot_stride);
  uint4* __restrict__ d4 = reinterpret_cast<uint4*>(packed) + d0;
  for (unsigned long long kb = k0; kb < k1; kb += (unsigned long long)TL_THREADS * TL_UNROLL) {
    uint4 v[TL_UNROLL];
#pragma unroll
    for (uint32_t u = 0; u < TL_UNROLL; ++u) {
      const unsigned long long k = kb + (unsigned long long)u * TL_THREADS + threadIdx.x;
      if (k < k1) v[u] = s4[k];
    }
#pragma unroll
    for (uint32_t u = 0; u < TL_UNROLL; ++u) {
      const unsigned long long k = kb + (unsigned long long)u * TL_THREADS + threadIdx.x;
      if (k < k1) d4[k] = v[u];
    }
  }
}

struct AlphaMergeArgs {
  const uint8_t* dec;                  // decoded triplet images, dec_stride apart, rows of aw3 bytes
  uint64_t dec_stride;
  uint32_t aw3;
  const int32_t* dec_status;           // of the decoded images
  const uint8_t* packed;               // raw planes at their offsets
  const unsigned long long* src;       // per slot: decoded image index, offset in packed, or the constant
  const uint8_t* kind;                 // per slot: 0 coded, 1 raw, 2 constant
  const uint32_t* tile_idx;
  uint32_t x0, y0, rw, rh;
  uint8_t* out;                        // the window's 4-byte pixels
  uint64_t out_pitch;
};

// Byte +3 of the window's pixels from slot i's tile, cut to the rectangle and
// the image; a coded slot whose decode failed is skipped.  quad: x0 and the
// tile's x origin are multiples of 4 and the window's rows 16-byte aligned, so
// a lane rewrites four pixels' alpha as one 16-byte read-modify-write (the
// colour bytes come back as they were); the group the window or the image ends
// in, and every other case, stores bytes.
template <int MODE>
__global__ __launch_bounds__(TL_THREADS) void alpha_merge(AlphaMergeArgs a, TileGrid q) {
  const uint32_t slot = blockIdx.x / q.bands, band = blockIdx.x % q.bands;
  const uint32_t kind = a.kind[slot];
  const unsigned long long src = a.src[slot];
  if (kind == 0 && a.dec_status[src] != 0) return;
  const uint32_t t = a.tile_idx[slot];
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  const TileCut c = tile_cut(t, q.nx, q.tw, q.th, band, q.rows_pb, a.x0, a.y0, a.rw, a.rh, q.w, q.h);
  if (c.empty) return;
  const uint32_t xa = c.xa, nxp = c.nxp, ya = c.ya, yb = c.yb;
  const bool cst = kind == 2;
  const uint32_t cval = (uint32_t)src & 255u;
  // the tile's plane: row pitch and first byte (unused for a constant)
  const uint32_t sp = kind == 0 ? a.aw3 : q.tw;
  const uint8_t* st = cst ? a.out : kind == 0 ? a.dec + src * a.dec_stride : a.packed + src;
  for (uint32_t y = ya + wave; y < yb; y += TL_WAVES) {
    const uint8_t* srow = st + (uint64_t)(y - c.ty0) * sp + (xa - c.tx0);
    uint8_t* drow = a.out + (uint64_t)(y - a.y0) * a.out_pitch + 4ull * (xa - a.x0);
    alpha_merge_row<MODE>(srow, drow, nxp, cst, cval, lane);
  }
}

namespace {
// Blocks per tile and rows per block for rows of row_bytes; false if the grid does not fit.
bool tile_bands(uint32_t slots, uint32_t th, uint64_t row_bytes, TileGrid& q) {
  return tl_bands(slots, th, row_bytes, q.bands, q.rows_pb);
}
// Pixels per block of the two per-pixel kernels.
bool px_chunks(uint32_t n, uint32_t npx, uint32_t& chunks, uint32_t& per) {
  per = TL_THREADS * TL_UNROLL * 8;
  chunks = (npx + per - 1) / per;
  return (uint64_t)n * chunks <= 0x7FFFFFFFull;
}
inline bool al(const void* p, uint64_t s, uint32_t a) { return tl_aligned(p, s, a); }
}  // namespace

int tiles_split_launch(void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t channels,
                       uint32_t tile_w, uint32_t tile_h, uint32_t nx, uint32_t ny, uint8_t* d_tiles,
                       uint64_t tile_stride) {
  TileGrid q{w, h, tile_w, tile_h, nx, 0, 0};
  const uint32_t n = nx * ny;
  if (!tile_bands(n, tile_h, (uint64_t)tile_w * channels, q)) return NICE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(n * q.bands), block(TL_THREADS);
  const bool rgba = channels == 4;
  if (rgba && (tile_w & 3u) == 0 && al(d_img, row_pitch, 16) && al(d_tiles, tile_stride, 16))
    hipLaunchKernelGGL(tiles_split<TL_QUAD>, grid, block, 0, st, d_img, row_pitch, channels, q, d_tiles, tile_stride);
  else if (rgba && al(d_img, row_pitch, 4) && al(d_tiles, tile_stride, 4))
    hipLaunchKernelGGL(tiles_split<TL_DWORD>, grid, block, 0, st, d_img, row_pitch, channels, q, d_tiles, tile_stride);
  else
    hipLaunchKernelGGL(tiles_split<TL_BYTES>, grid, block, 0, st, d_img, row_pitch, channels, q, d_tiles, tile_stride);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int tiles_merge_launch(void* stream, const uint8_t* d_tiles, uint64_t tile_stride, const uint64_t* d_src_off,
                       const uint32_t* d_tile_idx, const int32_t* d_slot_status, uint32_t n_slots, uint32_t w,
                       uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t nx, uint32_t ny, uint32_t x0, uint32_t y0,
                       uint32_t rw, uint32_t rh, uint32_t tile_channels, uint32_t out_channels, uint32_t fill,
                       uint8_t* d_out, uint64_t out_pitch) {
  if (n_slots == 0) return NICE_OK;
  TileGrid q{w, h, tile_w, tile_h, nx, 0, 0};
  if (!tile_bands(n_slots, tile_h, (uint64_t)tile_w * tile_channels, q)) return NICE_E_ARG;
  MergeArgs a{d_tiles, tile_stride, (const unsigned long long*)d_src_off, d_tile_idx, d_slot_status, nx * ny,
              x0, y0, rw, rh, tile_channels, out_channels, fill, d_out, out_pitch};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(n_slots * q.bands), block(TL_THREADS);
  const bool rgba = tile_channels == 4 && out_channels == 4 && !d_src_off;
  if (rgba && (tile_w & 3u) == 0 && (x0 & 3u) == 0 && al(d_tiles, tile_stride, 16) && al(d_out, out_pitch, 16))
    hipLaunchKernelGGL(tiles_merge<TL_QUAD>, grid, block, 0, st, a, q);
  else if (rgba && al(d_tiles, tile_stride, 4) && al(d_out, out_pitch, 4))
    hipLaunchKernelGGL(tiles_merge<TL_DWORD>, grid, block, 0, st, a, q);
  else
    hipLaunchKernelGGL(tiles_merge<TL_BYTES>, grid, block, 0, st, a, q);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int tiles_compare_launch(void* stream, const uint8_t* d_a, uint64_t stride_a, const uint8_t* d_b, uint64_t stride_b,
                         uint32_t channels, uint32_t n, uint32_t npx, const int32_t* d_status, uint8_t* d_kind) {
  uint32_t chunks, per;
  if (!px_chunks(n, npx, chunks, per)) return NICE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_kind, 0, n, st) != hipSuccess) return NICE_E_HIP;
  const int dword = channels == 4 && al(d_a, stride_a, 4) && al(d_b, stride_b, 4);
  hipLaunchKernelGGL(tiles_compare, dim3(n * chunks), dim3(TL_THREADS), 0, st, d_a, stride_a, d_b, stride_b, channels,
                     npx, chunks, per, dword, d_status, d_kind);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int tiles_store_raw_launch(void* stream, const uint8_t* d_tiles, uint64_t tile_stride, uint32_t channels, uint32_t n,
                           uint32_t npx, const uint8_t* d_kind, uint8_t* d_slots, uint64_t slot_stride,
                           uint64_t* d_len) {
  uint32_t chunks, per;
  if (!px_chunks(n, npx, chunks, per)) return NICE_E_ARG;
  hipLaunchKernelGGL(tiles_store_raw, dim3(n * chunks), dim3(TL_THREADS), 0, (hipStream_t)stream, d_tiles, tile_stride,
                     channels, npx, chunks, per, d_kind, d_slots, slot_stride, (unsigned long long*)d_len);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int tiles_scatter_status_launch(void* stream, const int32_t* d_st, const uint32_t* d_pos, uint32_t n, int32_t* d_out) {
  if (n == 0) return NICE_OK;
  hipLaunchKernelGGL(tiles_scatter_status, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_st, d_pos, n,
                     d_out);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int alpha_range_launch(void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t tile_w,
                       uint32_t tile_h, uint32_t nx, uint32_t ny, uint32_t* d_lo, uint32_t* d_hi) {
  TileGrid q{w, h, tile_w, tile_h, nx, 0, 0};
  const uint32_t n = nx * ny;
  if (!tile_bands(n, tile_h, 4ull * tile_w, q)) return NICE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_lo, 0xFF, 4ull * n, st) != hipSuccess) return NICE_E_HIP;   // (atomicMin brings it down to <= 255)
  if (hipMemsetAsync(d_hi, 0, 4ull * n, st) != hipSuccess) return NICE_E_HIP;
  const dim3 grid(n * q.bands), block(TL_THREADS);
  if (al(d_img, row_pitch, 16))
    hipLaunchKernelGGL(alpha_range<TL_QUAD>, grid, block, 0, st, d_img, row_pitch, q, d_lo, d_hi);
  else if (al(d_img, row_pitch, 4))
    hipLaunchKernelGGL(alpha_range<TL_DWORD>, grid, block, 0, st, d_img, row_pitch, q, d_lo, d_hi);
  else
    hipLaunchKernelGGL(alpha_range<TL_BYTES>, grid, block, 0, st, d_img, row_pitch, q, d_lo, d_hi);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int alpha_gather_launch(void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w, uint32_t h, uint32_t tile_w,
                        uint32_t tile_h, uint32_t nx, const uint32_t* d_list, uint32_t m, uint8_t* d_trip,
                        uint64_t trip_stride) {
  if (m == 0) return NICE_OK;
  TileGrid q{w, h, tile_w, tile_h, nx, 0, 0};
  const uint32_t aw3 = (tile_w + 2u) / 3u * 3u;
  if (!tile_bands(m, tile_h, aw3, q)) return NICE_E_ARG;
  hipLaunchKernelGGL(alpha_gather, dim3(m * q.bands), dim3(TL_THREADS), 0, (hipStream_t)stream, d_img, row_pitch, q,
                     d_list, aw3, d_trip, trip_stride);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int alpha_store_launch(void* stream, const uint8_t* d_trip, uint64_t trip_stride, uint32_t tile_w, uint32_t tile_h,
                       const uint32_t* d_list, uint32_t m, uint8_t* d_vk, uint64_t* d_mlen, uint8_t* d_slots,
                       uint64_t slot_stride, uint8_t* d_akind, uint64_t* d_alen) {
  if (m == 0) return NICE_OK;
  TileGrid q{0, 0, tile_w, tile_h, 0, 0, 0};
  const uint32_t aw3 = (tile_w + 2u) / 3u * 3u;
  if (!tile_bands(m, tile_h, tile_w, q)) return NICE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(alpha_verdict, dim3((m + 255) / 256), dim3(256), 0, st, d_list, m, tile_w * tile_h, d_vk,
                     (unsigned long long*)d_mlen, d_slots, slot_stride, d_akind, (unsigned long long*)d_alen);
  hipLaunchKernelGGL(alpha_store_raw, dim3(m * q.bands), dim3(TL_THREADS), 0, st, d_trip, trip_stride, aw3, q, d_vk,
                     d_slots, slot_stride);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int alpha_pack_launch(void* stream, const uint8_t* d_slots, uint64_t slot_stride, const uint64_t* d_mlen,
                      const uint32_t* d_list, uint32_t m, const uint64_t* d_off, uint8_t* d_packed, uint64_t packed_cap) {
  if (m == 0 || packed_cap < 16) return NICE_OK;
  const uint64_t chunks = (slot_stride / 16 + AL_PACK_GRANULES - 1) / AL_PACK_GRANULES;
  if ((uint64_t)m * chunks > 0x7FFFFFFFull) return NICE_E_ARG;
  hipLaunchKernelGGL(alpha_pack, dim3((uint32_t)(m * chunks)), dim3(TL_THREADS), 0, (hipStream_t)stream, d_slots,
                     slot_stride, (const unsigned long long*)d_mlen, d_list, (uint32_t)chunks,
                     (const unsigned long long*)d_off, d_packed, (unsigned long long)packed_cap);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int alpha_merge_launch(void* stream, const uint8_t* d_dec, uint64_t dec_stride, const int32_t* d_dec_status,
                       const uint8_t* d_packed, const uint64_t* d_src, const uint8_t* d_kind, const uint32_t* d_tile_idx,
                       uint32_t n_slots, uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t nx,
                       uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh, uint8_t* d_out, uint64_t out_pitch) {
  if (n_slots == 0) return NICE_OK;
  TileGrid q{w, h, tile_w, tile_h, nx, 0, 0};
  if (!tile_bands(n_slots, tile_h, 4ull * tile_w, q)) return NICE_E_ARG;
  AlphaMergeArgs a{d_dec, dec_stride, (tile_w + 2u) / 3u * 3u, d_dec_status, d_packed, (const unsigned long long*)d_src,
                   d_kind, d_tile_idx, x0, y0, rw, rh, d_out, out_pitch};
  const dim3 grid(n_slots * q.bands), block(TL_THREADS);
  if ((tile_w & 3u) == 0 && (x0 & 3u) == 0 && al(d_out, out_pitch, 16))
    hipLaunchKernelGGL(alpha_merge<TL_QUAD>, grid, block, 0, (hipStream_t)stream, a, q);
  else
    hipLaunchKernelGGL(alpha_merge<TL_BYTES>, grid, block, 0, (hipStream_t)stream, a, q);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

}  // namespace nice
