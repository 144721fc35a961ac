// nice_sets_tensor.hip -- image sets, tensor output (include/nice.h, "image
// sets: tensor output"): set_merge (nice_sets.hip) that converts as it stores.
// The slot tables, the bands, the per-block window descriptor and the cut of a
// tile to its window and image (tile_cut) are set_merge's.  New: every output
// element is fmaf(byte, scale[c], bias[c]) in binary32, stored as float32 or
// rounded to nearest even to float16 / bfloat16 (tensor_value); the window is
// planar or interleaved and may be mirrored.  A lane takes P = 1, 2, 4 or 8 consecutive pixels: it loads
// them as P dwords (dense 4-byte slots) or 3 P bytes (raw slots) and stores P
// elements per plane as one store of 4, 8 or 16 bytes; P is a field of the
// window descriptor, so one launch serves windows of different alignment (a
// wave-uniform branch).  A row with fewer than 64 groups shares its wave with
// the rows below it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nice.h"
#include "nice_internal.h"
#include "nice_sets_tensor.hpp"
#include "nice_tile_geom.hpp"
#include "nice_tiles.hpp"

namespace nice {

struct SetTensorArgs {
  const uint8_t* tiles;
  uint64_t tile_stride;
  const unsigned long long* src_off;   // non-null: slot i at tiles + src_off[i]
  const uint32_t* slot_win;
  const uint32_t* slot_tile;
  const int32_t* slot_status;          // non-null: a slot with a nonzero status is skipped
  const SetTensorWindow* wins;
  uint32_t n_wins;
  uint32_t tw, th, bands, rows_pb;
  uint32_t tc;                         // bytes per pixel in the slots
  uint32_t src_dwords;                 // the slots hold 4-byte pixels at 4-byte alignment: a pixel is one dword load
  uint32_t mode_cap;                   // the best mode the slots allow
  float scale[3], bias[3];
};

// The cut c of the tile at st -> window d.  A lane takes the group of
// P = 1 << LP pixels at image column P * g; a group that the tile, the window
// or the image cuts goes pixel by pixel.  LP > 0: P divides x0 (flipped: x0 + rw), the pitches and, with
// src_dwords, the tile width, and base and slots are aligned to match
// (set_tensor_window_mode, set_merge_tensor_launch).
template <int DT, int LAYOUT, int LP>
__device__ __forceinline__ void set_tensor_rows(const SetTensorArgs& a, const SetTensorWindow& d, const uint8_t* st,
                                                const TileCut& c) {
  using B = typename TensorElem<DT>::bits;
  constexpr uint32_t P = 1u << LP;
  constexpr uint32_t U = P == 8 ? TL_UNROLL / 2 : TL_UNROLL;   // at most 4 x 1 KiB of loads in flight per wave
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  const uint32_t tx0 = c.tx0, ty0 = c.ty0, xa = c.xa, ya = c.ya, yb = c.yb, xe = xa + c.nxp;
  const uint32_t gb = xa >> LP, ge = (xe + P - 1u) >> LP;   // the groups of the image row that hold [xa, xe)
  const RowShare rs = row_share(ge - gb);   // the lanes a row does not need take the rows below
  const uint32_t lpr = rs.lpr, rpw = rs.rpw, lx = lane & (lpr - 1u), ly = lane >> rs.ls;
  const bool flip = d.flip != 0;
  const uint32_t xlast = d.x0 + d.rw - 1u;   // the window's last image column
  B* const out = reinterpret_cast<B*>(d.out);
  // channel ch of the pixel px
  const auto elem = [&](uint32_t px, uint32_t ch) {
    return tensor_value<DT>((float)((px >> (8u * ch)) & 255u), a.scale[ch], a.bias[ch]);
  };
  // (the unrolled steps go along the row; taking them down the rows where a row
  // is one step measured 8 % slower on the crop batch, at 12 VGPRs more)
  for (uint32_t y = ya + wave * rpw + ly; y < yb; y += TL_WAVES * rpw) {
    const uint8_t* srow = st + (uint64_t)(y - ty0) * a.tw * a.tc;   // pixel x of the row at srow + (x - tx0) * tc
    B* const orow = out + (uint64_t)(y - d.y0) * d.row_pitch;
    for (uint32_t g0 = gb; g0 < ge; g0 += lpr * U) {
      uint32_t v[U][P];
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        const uint32_t g = g0 + lpr * u + lx;
        if (g < ge) {
          const uint32_t x = g << LP;
          const bool whole = x >= xa && x + P <= xe;
          if (a.src_dwords) {
            if (P == 1 || !whole) {   // (only the pixels inside [xa, xe) are read)
#pragma unroll
              for (uint32_t k = 0; k < P; ++k)
                if (x + k >= xa && x + k < xe) v[u][k] = ld32(srow + 4ull * (x + k - tx0));
            } else if constexpr (P == 2) {
              const uint2 q = *reinterpret_cast<const uint2*>(srow + 4ull * (x - tx0));
              v[u][0] = q.x;
              v[u][1] = q.y;
            } else if constexpr (P >= 4) {
#pragma unroll
              for (uint32_t k = 0; k < P; k += 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(srow + 4ull * (x + k - tx0));
                v[u][k] = q.x;
                v[u][k + 1] = q.y;
                v[u][k + 2] = q.z;
                v[u][k + 3] = q.w;
              }
            }
          } else {
#pragma unroll
            for (uint32_t k = 0; k < P; ++k)
              if (x + k >= xa && x + k < xe) v[u][k] = ld_px_bytes(srow + (uint64_t)(x + k - tx0) * a.tc, 3u, 0u);
          }
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        const uint32_t g = g0 + lpr * u + lx;
        if (g < ge) {
          const uint32_t x = g << LP;
          bool whole = false;
          if constexpr (P > 1) whole = x >= xa && x + P <= xe;
          if constexpr (P > 1) if (whole) {
            // output columns xo .. xo + P - 1, a multiple of P; mirrored, they take the group's pixels from the last
            const uint32_t xo = flip ? xlast + 1u - P - x : x - d.x0;
            uint32_t q[P];
#pragma unroll
            for (uint32_t k = 0; k < P; ++k) q[k] = flip ? v[u][P - 1u - k] : v[u][k];
            st_group<B, P, LAYOUT>(orow, d.plane_pitch, xo, [&](uint32_t k, uint32_t ch) { return elem(q[k], ch); });
          }
          if (!whole) {
#pragma unroll
            for (uint32_t k = 0; k < P; ++k) {
              if (x + k >= xa && x + k < xe) {
                const uint32_t xo = flip ? xlast - (x + k) : x + k - d.x0;
                st_one<B, LAYOUT>(orow, d.plane_pitch, xo, [&](uint32_t ch) { return elem(v[u][k], ch); });
              }
            }
          }
        }
      }
    }
  }
}

// Slots -> windows, as set_merge: slot i holds tile slot_tile[i] of the image
// of window slot_win[i]; its part inside that window's rectangle and image
// goes to the window's elements, and nothing else is written.
template <int DT, int LAYOUT>
__global__ __launch_bounds__(TL_THREADS) void set_merge_tensor(SetTensorArgs a) {
  const uint32_t slot = blockIdx.x / a.bands, band = blockIdx.x % a.bands;
  if (a.slot_status && a.slot_status[slot] != 0) return;
  const uint32_t wi = a.slot_win[slot];
  if (wi >= a.n_wins) return;
  const SetTensorWindow d = a.wins[wi];
  const uint32_t t = a.slot_tile[slot];
  if (t >= d.n_tiles) return;
  // the tile's pixels inside the rectangle and the image
  const TileCut c = tile_cut(t, d.nx, a.tw, a.th, band, a.rows_pb, d.x0, d.y0, d.rw, d.rh, d.w, d.h);
  if (c.empty) return;
  const uint8_t* st = a.tiles + (a.src_off ? (uint64_t)a.src_off[slot] : (uint64_t)slot * a.tile_stride);
  const uint32_t mode = min(d.mode, a.mode_cap);
  if (mode == 3u) {   // (float32: the launch caps the mode at 2, 16 bytes per store)
    if constexpr (DT != (int)NICE_TENSOR_F32)
      set_tensor_rows<DT, LAYOUT, 3>(a, d, st, c);
  } else if (mode == 2u) {
    set_tensor_rows<DT, LAYOUT, 2>(a, d, st, c);
  } else if (mode == 1u) {
    set_tensor_rows<DT, LAYOUT, 1>(a, d, st, c);
  } else {
    set_tensor_rows<DT, LAYOUT, 0>(a, d, st, c);
  }
}

uint32_t set_tensor_elem_bytes(uint32_t dtype) {
  return dtype == NICE_TENSOR_F32 ? 4u : (dtype == NICE_TENSOR_F16 || dtype == NICE_TENSOR_BF16) ? 2u : 0u;
}

namespace {
// the widest store is 16 bytes: 4 float32 or 8 16-bit elements
uint32_t max_mode(uint32_t dtype) { return dtype == NICE_TENSOR_F32 ? 2u : 3u; }
}  // namespace

// (plane_pitch: 0 for an interleaved window; the groups count from x0, mirrored from x0 + rw)
uint32_t set_tensor_window_mode(const void* d_out, uint64_t row_pitch, uint64_t plane_pitch, uint32_t x0, uint32_t rw,
                                bool flip, uint32_t dtype) {
  return vector_mode((uintptr_t)d_out, set_tensor_elem_bytes(dtype), row_pitch, plane_pitch, flip ? (uint64_t)x0 + rw : x0,
                     max_mode(dtype));
}

int set_merge_tensor_launch(void* stream, const uint8_t* d_tiles, uint64_t tile_stride, const uint64_t* d_src_off,
                            const uint32_t* d_slot_win, const uint32_t* d_slot_tile, const int32_t* d_slot_status,
                            uint32_t n_slots, const SetTensorWindow* d_wins, uint32_t n_wins, uint32_t tile_w,
                            uint32_t tile_h, uint32_t tile_channels, uint32_t dtype, uint32_t layout, const float* scale,
                            const float* bias) {
  if (n_slots == 0) return NICE_OK;
  SetTensorArgs a{d_tiles, tile_stride, (const unsigned long long*)d_src_off, d_slot_win, d_slot_tile, d_slot_status,
                  d_wins, n_wins, tile_w, tile_h, 0, 0, tile_channels, 0, max_mode(dtype),
                  {scale[0], scale[1], scale[2]}, {bias[0], bias[1], bias[2]}};
  if (!tl_bands(n_slots, tile_h, (uint64_t)tile_w * tile_channels, a.bands, a.rows_pb)) return NICE_E_ARG;
  if (tile_channels == 4 && !d_src_off && tl_aligned(d_tiles, tile_stride, 4)) {
    // dword pixels; a lane's P of them are one load where the tile rows are aligned to 4 P bytes
    a.src_dwords = 1;
    a.mode_cap = 0;
    for (uint32_t lp = 1; lp <= max_mode(dtype); ++lp) {
      if (!tl_aligned(d_tiles, tile_stride, std::min(4u << lp, 16u)) || (tile_w & ((1u << lp) - 1u))) break;
      a.mode_cap = lp;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(n_slots * a.bands), block(TL_THREADS);
  const int rc = tensor_dispatch(dtype, layout, [&](auto dt, auto lay) {
    hipLaunchKernelGGL((set_merge_tensor<decltype(dt)::value, decltype(lay)::value>), grid, block, 0, st, a);
  });
  return rc ? rc : hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

}  // namespace nice
