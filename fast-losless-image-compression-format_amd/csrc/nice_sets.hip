// nice_sets.hip -- image sets (include/nice.h, "image sets"): the copies between
// many pitched images of different sizes and one dense array of equally sized
// tiles.  The design is nice_tiles.hip's: a block takes a band of rows of one
// tile, a wave one row at a time, a lane one pixel (or four, 16 bytes);
// everything but the lane's column is wave-uniform and a lane's loads are
// issued before its stores.  New here: the image (split) or the window (merge)
// a block works for is found once per block from a small descriptor table, by
// wave-uniform loads, and the move mode is a field of that descriptor, so one
// launch serves members that need different modes (a wave-uniform branch).
// The set's alpha batch (range, gather, merge) follows the colour kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nice.h"
#include "nice_internal.h"
#include "nice_tile_geom.hpp"
#include "nice_tiles.hpp"

namespace nice {

struct SetSplitArgs {
  const SetImage* imgs;
  uint32_t K, C;
  uint32_t tw, th, bands, rows_pb;
  uint32_t mode_cap;   // the best mode the tile array allows
  uint8_t* tiles;
  uint64_t tile_stride;
};

// Rows [r0, r1) of tile (tx, ty) of image d -> dt.  Tile position (g, r) takes
// the image pixel at the clamped coordinate: every load is inside the image,
// every store inside the tile.
template <int MODE>
__device__ __forceinline__ void set_split_rows(const SetImage& d, uint32_t C, uint32_t tw, uint32_t x0, uint32_t y0,
                                               uint32_t r0, uint32_t r1, uint8_t* dt) {
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  const uint32_t xl = d.w - 1;
  for (uint32_t r = r0 + wave; r < r1; r += TL_WAVES) {
    const uint32_t y = min(y0 + r, d.h - 1);
    const uint8_t* srow = d.img + (uint64_t)y * d.pitch;
    uint8_t* drow = dt + (uint64_t)r * tw * C;
    if (MODE == TL_QUAD) {
      const uint32_t G = tw >> 2;
      for (uint32_t g0 = 0; g0 < G; g0 += 64u * TL_UNROLL) {
        uint4 v[TL_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) {
          const uint32_t g = g0 + 64u * u + lane;
          if (g < G) {
            const uint32_t x = x0 + 4u * g;
            if (x + 4u <= d.w) {
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
      for (uint32_t g0 = 0; g0 < tw; g0 += 64u * TL_UNROLL) {
        uint32_t v[TL_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) {
          const uint32_t g = g0 + 64u * u + lane;
          if (g < tw) {
            const uint8_t* s = srow + (uint64_t)min(x0 + g, xl) * C;
            v[u] = MODE == TL_DWORD ? ld32(s) : ld_px_bytes(s, C, 0u);
          }
        }
#pragma unroll
        for (uint32_t u = 0; u < TL_UNROLL; ++u) {
          const uint32_t g = g0 + 64u * u + lane;
          if (g < tw) {
            if (MODE == TL_DWORD) *reinterpret_cast<uint32_t*>(drow + 4ull * g) = v[u];
            else st_px_bytes(drow + (uint64_t)g * C, C, v[u]);
          }
        }
      }
    }
  }
}

// The image of global tile gt (wave-uniform): the last one whose `first` is not
// above that tile (first[0] == 0), found by a binary search of the descriptor
// table as pack_copy searches the offsets: log2(K) dependent scalar loads.
__device__ __forceinline__ uint32_t set_image_of(const SetImage* imgs, uint32_t K, uint32_t gt) {
  uint32_t lo = 0, hi = K;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (imgs[mid].first <= gt) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Images -> tiles.  Block b works on global tile b / bands of its image
// (set_image_of: once per block of about 32 KiB moved).
__global__ __launch_bounds__(TL_THREADS) void set_split(SetSplitArgs a) {
  const uint32_t gt = blockIdx.x / a.bands, band = blockIdx.x % a.bands;
  const SetImage d = a.imgs[set_image_of(a.imgs, a.K, gt)];
  const uint32_t t = gt - d.first;
  const uint32_t ty = t / d.nx, tx = t % d.nx;
  const uint32_t r0 = band * a.rows_pb, r1 = min(r0 + a.rows_pb, a.th);
  uint8_t* dt = a.tiles + (uint64_t)gt * a.tile_stride;
  const uint32_t mode = min(d.mode, a.mode_cap);
  if (mode == TL_QUAD) set_split_rows<TL_QUAD>(d, a.C, a.tw, tx * a.tw, ty * a.th, r0, r1, dt);
  else if (mode == TL_DWORD) set_split_rows<TL_DWORD>(d, a.C, a.tw, tx * a.tw, ty * a.th, r0, r1, dt);
  else set_split_rows<TL_BYTES>(d, a.C, a.tw, tx * a.tw, ty * a.th, r0, r1, dt);
}

struct SetMergeArgs {
  const uint8_t* tiles;
  uint64_t tile_stride;
  const unsigned long long* src_off;   // non-null: slot i at tiles + src_off[i]
  const uint32_t* slot_win;
  const uint32_t* slot_tile;
  const int32_t* slot_status;          // non-null: a slot with a nonzero status is skipped
  const SetWindow* wins;
  uint32_t n_wins;
  uint32_t tw, th, bands, rows_pb;
  uint32_t tc, oc, fill;               // bytes per pixel in the slots, in the windows; byte +3 when tc == 3
  uint32_t mode_cap;                   // the best mode the slots allow
};

// The cut c of the tile at st -> window d.
template <int MODE>
__device__ __forceinline__ void set_merge_rows(const SetMergeArgs& a, const SetWindow& d, const uint8_t* st,
                                               const TileCut& c) {
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  const uint32_t tx0 = c.tx0, ty0 = c.ty0, xa = c.xa, nxp = c.nxp, ya = c.ya, yb = c.yb;
  for (uint32_t y = ya + wave; y < yb; y += TL_WAVES) {
    const uint8_t* srow = st + ((uint64_t)(y - ty0) * a.tw + (xa - tx0)) * a.tc;
    uint8_t* drow = d.out + (uint64_t)(y - d.y0) * d.pitch + (uint64_t)(xa - d.x0) * a.oc;
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
            uint8_t* o = drow + 16ull * g;
            if (4u * g + 4u <= nxp) {
              *reinterpret_cast<uint4*>(o) = v[u];
            } else {   // the window or the image ends inside this group
              const uint32_t k = nxp - 4u * g;   // 1..3 pixels
              *reinterpret_cast<uint32_t*>(o) = v[u].x;
              if (k > 1) *reinterpret_cast<uint32_t*>(o + 4) = v[u].y;
              if (k > 2) *reinterpret_cast<uint32_t*>(o + 8) = v[u].z;
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

// Slots -> windows.  Slot i holds tile slot_tile[i] of the image of window
// slot_win[i]; its part inside that window's rectangle and image (no padding is
// ever written) goes to out + (y - y0) * pitch + (x - x0) * oc of the window.
__global__ __launch_bounds__(TL_THREADS) void set_merge(SetMergeArgs a) {
  const uint32_t slot = blockIdx.x / a.bands, band = blockIdx.x % a.bands;
  if (a.slot_status && a.slot_status[slot] != 0) return;
  const uint32_t wi = a.slot_win[slot];
  if (wi >= a.n_wins) return;
  const SetWindow d = a.wins[wi];
  const uint32_t t = a.slot_tile[slot];
  if (t >= d.n_tiles) return;
  // the tile's pixels inside the rectangle and the image
  const TileCut c = tile_cut(t, d.nx, a.tw, a.th, band, a.rows_pb, d.x0, d.y0, d.rw, d.rh, d.w, d.h);
  if (c.empty) return;
  const uint8_t* st = a.tiles + (a.src_off ? (uint64_t)a.src_off[slot] : (uint64_t)slot * a.tile_stride);
  const uint32_t mode = min(d.mode, a.mode_cap);
  if (mode == TL_QUAD) set_merge_rows<TL_QUAD>(a, d, st, c);
  else if (mode == TL_DWORD) set_merge_rows<TL_DWORD>(a, d, st, c);
  else set_merge_rows<TL_BYTES>(a, d, st, c);
}

// ---- alpha (include/nice.h, "image sets: alpha") -------------------------------
// The set forms of nice_tiles.hip's alpha_range, alpha_gather and alpha_merge:
// the rows are theirs (nice_tiles.hpp); the image or the window comes from the
// descriptor table, and with it the mode.

struct SetAlphaRangeArgs {
  const SetImage* imgs;
  uint32_t K;
  uint32_t tw, th, bands, rows_pb;
  uint32_t* lo;
  uint32_t* hi;
};

template <int MODE>
__device__ __forceinline__ void set_alpha_range_rows(const SetImage& d, uint32_t xs, uint32_t xe, uint32_t ys, uint32_t ye,
                                                     uint32_t* lo, uint32_t* hi) {
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  uint32_t mn = 255u, mx = 0u;
  for (uint32_t y = ys + wave; y < ye; y += TL_WAVES)
    alpha_range_row<MODE>(d.img + (uint64_t)y * d.pitch, d.w, xs, xe, lane, mn, mx);
  alpha_range_commit(mn, mx, lane, lo, hi);
}

// lo[g] / hi[g] = min / max of byte +3 over global tile g (preset to 255 / 0).
// Only pixels inside the tile's image are read.
__global__ __launch_bounds__(TL_THREADS) void set_alpha_range(SetAlphaRangeArgs a) {
  const uint32_t gt = blockIdx.x / a.bands, band = blockIdx.x % a.bands;
  const SetImage d = a.imgs[set_image_of(a.imgs, a.K, gt)];
  const uint32_t t = gt - d.first;
  const uint32_t ty = t / d.nx, tx = t % d.nx;
  const uint32_t xs = tx * a.tw, xe = min(xs + a.tw, d.w);
  const uint32_t ys = ty * a.th + band * a.rows_pb;
  const uint32_t ye = min(ty * a.th + min((band + 1) * a.rows_pb, a.th), d.h);
  if (d.mode == TL_QUAD) set_alpha_range_rows<TL_QUAD>(d, xs, xe, ys, ye, &a.lo[gt], &a.hi[gt]);
  else if (d.mode == TL_DWORD) set_alpha_range_rows<TL_DWORD>(d, xs, xe, ys, ye, &a.lo[gt], &a.hi[gt]);
  else set_alpha_range_rows<TL_BYTES>(d, xs, xe, ys, ye, &a.lo[gt], &a.hi[gt]);
}

struct SetAlphaGatherArgs {
  const SetImage* imgs;
  uint32_t K;
  uint32_t tw, th, bands, rows_pb;
  const uint32_t* list;
  uint32_t aw3;
  uint8_t* trip;
  uint64_t trip_stride;
};

// Triplet image of global tile list[i] at trip + i * trip_stride (bytes, as alpha_gather).
__global__ __launch_bounds__(TL_THREADS) void set_alpha_gather(SetAlphaGatherArgs a) {
  const uint32_t i = blockIdx.x / a.bands, band = blockIdx.x % a.bands;
  const uint32_t gt = a.list[i];
  const SetImage d = a.imgs[set_image_of(a.imgs, a.K, gt)];
  const uint32_t t = gt - d.first;
  const uint32_t ty = t / d.nx, tx = t % d.nx;
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  const uint32_t r0 = band * a.rows_pb, r1 = min(r0 + a.rows_pb, a.th);
  const uint32_t xs = tx * a.tw, xl = d.w - 1;
  uint8_t* dt = a.trip + (uint64_t)i * a.trip_stride;
  for (uint32_t r = r0 + wave; r < r1; r += TL_WAVES) {
    const uint8_t* srow = d.img + (uint64_t)min(ty * a.th + r, d.h - 1) * d.pitch;
    alpha_gather_row(srow, dt + (uint64_t)r * a.aw3, a.aw3, xs, a.tw, xl, lane);
  }
}

struct SetAlphaMergeArgs {
  const uint8_t* dec;                  // decoded triplet images, dec_stride apart, rows of aw3 bytes
  uint64_t dec_stride;
  uint32_t aw3;
  const int32_t* dec_status;           // of the decoded images
  const uint8_t* packed;               // raw planes at their offsets
  const unsigned long long* src;       // per slot: decoded image index, offset in packed, or the constant
  const uint8_t* kind;                 // per slot: 0 coded, 1 raw, 2 constant
  const uint32_t* slot_win;
  const uint32_t* slot_tile;
  const SetWindow* wins;
  uint32_t n_wins;
  uint32_t tw, th, bands, rows_pb;
  uint32_t mode_cap;                   // TL_QUAD where tw % 4 == 0, else TL_BYTES
};

template <int MODE>
__device__ __forceinline__ void set_alpha_merge_rows(const SetWindow& d, const uint8_t* st, uint32_t sp, bool cst,
                                                     uint32_t cval, const TileCut& c) {
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  for (uint32_t y = c.ya + wave; y < c.yb; y += TL_WAVES) {
    const uint8_t* srow = st + (uint64_t)(y - c.ty0) * sp + (c.xa - c.tx0);
    uint8_t* drow = d.out + (uint64_t)(y - d.y0) * d.pitch + 4ull * (c.xa - d.x0);
    alpha_merge_row<MODE>(srow, drow, c.nxp, cst, cval, lane);
  }
}

// Byte +3 of the windows' pixels.  Slot i holds tile slot_tile[i] of the image
// of window slot_win[i], cut to that window and the image exactly as set_merge
// cuts it.  Skipped: a coded slot whose decode failed, a window index >= n_wins,
// a tile index outside its image.  The quad mode is the window's own (16-byte
// base and pitch, x0 % 4 == 0) where tw % 4 == 0: then xa and the row are
// 16-byte aligned.
__global__ __launch_bounds__(TL_THREADS) void set_alpha_merge(SetAlphaMergeArgs a) {
  const uint32_t slot = blockIdx.x / a.bands, band = blockIdx.x % a.bands;
  const uint32_t kind = a.kind[slot];
  const unsigned long long src = a.src[slot];
  if (kind == 0 && a.dec_status[src] != 0) return;
  const uint32_t wi = a.slot_win[slot];
  if (wi >= a.n_wins) return;
  const SetWindow d = a.wins[wi];
  const uint32_t t = a.slot_tile[slot];
  if (t >= d.n_tiles) return;
  const TileCut c = tile_cut(t, d.nx, a.tw, a.th, band, a.rows_pb, d.x0, d.y0, d.rw, d.rh, d.w, d.h);
  if (c.empty) return;
  const bool cst = kind == 2;
  const uint32_t cval = (uint32_t)src & 255u;
  // the tile's plane: row pitch and first byte (unused for a constant)
  const uint32_t sp = kind == 0 ? a.aw3 : a.tw;
  const uint8_t* st = cst ? d.out : kind == 0 ? a.dec + src * a.dec_stride : a.packed + src;
  if (min(d.mode, a.mode_cap) == TL_QUAD)
    set_alpha_merge_rows<TL_QUAD>(d, st, sp, cst, cval, c);
  else
    set_alpha_merge_rows<TL_BYTES>(d, st, sp, cst, cval, c);
}

namespace {
static_assert(TL_BYTES == 0 && TL_DWORD == 1 && TL_QUAD == 2, "byte_mode's values");
// the best mode a base and its pitch (or stride) allow on their own
uint32_t mode_of(const void* p, uint64_t s) { return byte_mode((uintptr_t)p, s, 0); }
}  // namespace

uint32_t set_image_mode(const uint8_t* d_img, uint64_t row_pitch) { return mode_of(d_img, row_pitch); }

uint32_t set_window_mode(const uint8_t* d_out, uint64_t out_pitch, uint32_t x0) {
  return byte_mode((uintptr_t)d_out, out_pitch, x0);
}

int set_split_launch(void* stream, const SetImage* d_imgs, uint32_t K, uint32_t n, uint32_t channels, uint32_t tile_w,
                     uint32_t tile_h, uint8_t* d_tiles, uint64_t tile_stride) {
  SetSplitArgs a{d_imgs, K, channels, tile_w, tile_h, 0, 0, TL_BYTES, d_tiles, tile_stride};
  if (!tl_bands(n, tile_h, (uint64_t)tile_w * channels, a.bands, a.rows_pb)) return NICE_E_ARG;
  if (channels == 4) {
    a.mode_cap = mode_of(d_tiles, tile_stride);
    if (a.mode_cap == TL_QUAD && (tile_w & 3u) != 0) a.mode_cap = TL_DWORD;
  }
  hipLaunchKernelGGL(set_split, dim3(n * a.bands), dim3(TL_THREADS), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int set_merge_launch(void* stream, const uint8_t* d_tiles, uint64_t tile_stride, const uint64_t* d_src_off,
                     const uint32_t* d_slot_win, const uint32_t* d_slot_tile, const int32_t* d_slot_status,
                     uint32_t n_slots, const SetWindow* d_wins, uint32_t n_wins, uint32_t tile_w, uint32_t tile_h,
                     uint32_t tile_channels, uint32_t out_channels, uint32_t fill) {
  if (n_slots == 0) return NICE_OK;
  SetMergeArgs a{d_tiles, tile_stride, (const unsigned long long*)d_src_off, d_slot_win, d_slot_tile, d_slot_status,
                 d_wins, n_wins, tile_w, tile_h, 0, 0, tile_channels, out_channels, fill, TL_BYTES};
  if (!tl_bands(n_slots, tile_h, (uint64_t)tile_w * tile_channels, a.bands, a.rows_pb)) return NICE_E_ARG;
  if (tile_channels == 4 && out_channels == 4 && !d_src_off) {
    a.mode_cap = mode_of(d_tiles, tile_stride);
    if (a.mode_cap == TL_QUAD && (tile_w & 3u) != 0) a.mode_cap = TL_DWORD;
  }
  hipLaunchKernelGGL(set_merge, dim3(n_slots * a.bands), dim3(TL_THREADS), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int set_alpha_range_launch(void* stream, const SetImage* d_imgs, uint32_t K, uint32_t n, uint32_t tile_w,
                           uint32_t tile_h, uint32_t* d_lo, uint32_t* d_hi) {
  SetAlphaRangeArgs a{d_imgs, K, tile_w, tile_h, 0, 0, d_lo, d_hi};
  if (!tl_bands(n, tile_h, 4ull * tile_w, a.bands, a.rows_pb)) return NICE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_lo, 0xFF, 4ull * n, st) != hipSuccess) return NICE_E_HIP;   // (atomicMin brings it down to <= 255)
  if (hipMemsetAsync(d_hi, 0, 4ull * n, st) != hipSuccess) return NICE_E_HIP;
  hipLaunchKernelGGL(set_alpha_range, dim3(n * a.bands), dim3(TL_THREADS), 0, st, a);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int set_alpha_gather_launch(void* stream, const SetImage* d_imgs, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                            const uint32_t* d_list, uint32_t m, uint8_t* d_trip, uint64_t trip_stride) {
  if (m == 0) return NICE_OK;
  const uint32_t aw3 = (tile_w + 2u) / 3u * 3u;
  SetAlphaGatherArgs a{d_imgs, K, tile_w, tile_h, 0, 0, d_list, aw3, d_trip, trip_stride};
  if (!tl_bands(m, tile_h, aw3, a.bands, a.rows_pb)) return NICE_E_ARG;
  hipLaunchKernelGGL(set_alpha_gather, dim3(m * a.bands), dim3(TL_THREADS), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int set_alpha_merge_launch(void* stream, const uint8_t* d_dec, uint64_t dec_stride, const int32_t* d_dec_status,
                           const uint8_t* d_packed, const uint64_t* d_src, const uint8_t* d_kind,
                           const uint32_t* d_slot_win, const uint32_t* d_slot_tile, uint32_t n_slots,
                           const SetWindow* d_wins, uint32_t n_wins, uint32_t tile_w, uint32_t tile_h) {
  if (n_slots == 0) return NICE_OK;
  SetAlphaMergeArgs a{d_dec, dec_stride, (tile_w + 2u) / 3u * 3u, d_dec_status, d_packed, (const unsigned long long*)d_src,
                      d_kind, d_slot_win, d_slot_tile, d_wins, n_wins, tile_w, tile_h, 0, 0,
                      (tile_w & 3u) == 0 ? (uint32_t)TL_QUAD : (uint32_t)TL_BYTES};
  if (!tl_bands(n_slots, tile_h, 4ull * tile_w, a.bands, a.rows_pb)) return NICE_E_ARG;
  hipLaunchKernelGGL(set_alpha_merge, dim3(n_slots * a.bands), dim3(TL_THREADS), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

}  // namespace nice
