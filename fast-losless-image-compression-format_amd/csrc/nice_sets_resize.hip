// nice_sets_resize.hip -- image sets, resized tensor output (include/nice.h,
// "image sets: resized tensor output"): the windows of a set, each resampled to
// one out_h x out_w by fixed-point bilinear taps (nice_resize.hpp), converted
// and stored as the tensor merge stores (nice_sets_tensor.hip).  A tap near a
// tile edge needs two or four slots, so the kernel is output-centric: a block
// is a band of output rows of one window, and a source pixel's slot is found
// by arithmetic, slot_first + (ty - ty0) * ntx + (tx - tx0).  Whether a slot is
// dense (dwords) or raw (3 bytes per pixel) is data (src[p]), not the launch's.
// A lane owns P = 1, 2 or 4 consecutive output columns: their positions are
// computed once per block and kept packed in registers; for every row of its
// band it loads the 4 P taps, then stores P elements per plane as one store of
// 4, 8 or 16 bytes (float32) or 4 or 8 bytes (the 16-bit types).  P is a field of the window descriptor (a wave-uniform
// branch); a row with fewer than 64 groups shares its wave with the rows below.
// No LDS: neighbouring lanes read neighbouring or identical dwords, and the
// rows of a band re-read their source rows from the cache.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nice.h"
#include "nice_internal.h"
#include "nice_resize.hpp"
#include "nice_sets_tensor.hpp"
#include "nice_slot_plan.hpp"
#include "nice_tile_geom.hpp"
#include "nice_tiles.hpp"

namespace nice {

constexpr uint32_t RS_ROWS = 32;    // output rows per block
// a lane owns at most four columns (16 taps in flight, stores of 16 bytes in float32 and 8 in the
// 16-bit types): eight cost 50 VGPRs more and a wave per SIMD
constexpr uint32_t RS_MAX_MODE = 2;

struct SetResizeArgs {
  const uint8_t* tiles;
  uint64_t tile_stride;
  const uint8_t* packed;
  const unsigned long long* src;       // per position: kind and value (slot_position_sources)
  const int32_t* slot_status;          // non-null: an element with a tap in a slot of nonzero status is not written
  const SetResizeWindow* wins;
  uint32_t tw, th, ow, oh, bands;
  float scale[3], bias[3];
};

// a column's taps, packed: bits 0-13 the column of i0 inside its tile, 14-21
// the weight of i1, 22 whether i1 is the next pixel
constexpr uint32_t RS_CX = 0x3FFFu, RS_F_SHIFT = 14, RS_STEP_SHIFT = 22;

// Output rows [ya, yb) of window d.  A lane takes the group of P = 1 << LP
// output columns at P * g; the group the row ends in, and a group with an
// element that is not to be written, goes element by element.  LP > 0: base
// and pitches are aligned to match (set_resize_window_mode).
template <int DT, int LAYOUT, int LP>
__device__ __forceinline__ void set_resize_rows(const SetResizeArgs& a, const SetResizeWindow& d, uint32_t ya,
                                                uint32_t yb) {
  using B = typename TensorElem<DT>::bits;
  constexpr uint32_t P = 1u << LP;
  const uint32_t lane = threadIdx.x & 63u, wave = tl_wave();
  const uint32_t G = (a.ow + P - 1u) >> LP;   // the groups of a row
  const RowShare rs = row_share(G);   // the lanes a row does not need take the rows below
  const uint32_t lpr = rs.lpr, rpw = rs.rpw, lx = lane & (lpr - 1u), ly = lane >> rs.ls;
  B* const out = reinterpret_cast<B*>(d.out);
  const float scale[3] = {in_vgpr(a.scale[0]), in_vgpr(a.scale[1]), in_vgpr(a.scale[2])};
  const float bias[3] = {in_vgpr(a.bias[0]), in_vgpr(a.bias[1]), in_vgpr(a.bias[2])};
  const uint64_t plane_pitch = in_vgpr64(d.plane_pitch);
  const auto slot = [&](uint32_t p) { return slot_source(a.src, a.slot_status, a.tiles, a.tile_stride, a.packed, p); };
  for (uint32_t g = lx; g < G; g += lpr) {
    const uint32_t x = g << LP;
    // the columns' positions, once per block: the slot column of i0, and the rest packed
    uint32_t sc[P], cw[P];
#pragma unroll
    for (uint32_t k = 0; k < P; ++k) {
      sc[k] = 0;
      cw[k] = 0;
      if (x + k < a.ow) {
        const ResizePos c = resize_pos(d.flip ? a.ow - 1u - (x + k) : x + k, d.rw, a.ow);
        const uint32_t xs = d.x0 + c.i0, tx = xs / a.tw;
        sc[k] = tx - d.tx0;
        cw[k] = (xs - tx * a.tw) | (c.f << RS_F_SHIFT) | ((c.i1 != c.i0 ? 1u : 0u) << RS_STEP_SHIFT);
      }
    }
    for (uint32_t y = ya + wave * rpw + ly; y < yb; y += TL_WAVES * rpw) {
      const ResizePos r = resize_pos(y, d.rh, a.oh);
      const uint32_t ys = d.y0 + r.i0, ty = ys / a.th;
      const uint32_t cy0 = ys - ty * a.th;
      uint32_t cy1 = cy0, tr1 = ty - d.ty0;
      if (r.i1 != r.i0 && ++cy1 == a.th) {   // j1 is the first row of the tile below
        cy1 = 0;
        ++tr1;
      }
      const uint32_t p0 = d.slot_first + (ty - d.ty0) * d.ntx, p1 = d.slot_first + tr1 * d.ntx;
      const uint32_t o0 = cy0 * a.tw, o1 = cy1 * a.tw;
      // loads: the four taps of every column of the group (a column past the row's end reads as column 0 does
      // and is never stored); the slots are looked up without branches, a tile edge or not
      uint32_t v[P][4];
      uint32_t okm = 0;   // bit k: column k of the group is to be written
#pragma unroll
      for (uint32_t k = 0; k < P; ++k) {
        const uint32_t cx0 = cw[k] & RS_CX;
        uint32_t cx1 = cx0 + ((cw[k] >> RS_STEP_SHIFT) & 1u);
        const uint32_t wrap = cx1 == a.tw ? 1u : 0u;   // i1 is the first column of the tile to the right
        cx1 = wrap ? 0u : cx1;
        const uint32_t sc1 = sc[k] + wrap;
        const SlotSource s00 = slot(p0 + sc[k]), s01 = slot(p0 + sc1), s10 = slot(p1 + sc[k]), s11 = slot(p1 + sc1);
        if ((s00.bpp & s01.bpp & s10.bpp & s11.bpp) == 4u) {   // all dense: four dwords
          v[k][0] = ld32(s00.base + 4ull * (o0 + cx0));
          v[k][1] = ld32(s01.base + 4ull * (o0 + cx1));
          v[k][2] = ld32(s10.base + 4ull * (o1 + cx0));
          v[k][3] = ld32(s11.base + 4ull * (o1 + cx1));
          okm |= (x + k < a.ow ? 1u : 0u) << k;
        } else if (min(min(s00.bpp, s01.bpp), min(s10.bpp, s11.bpp)) != 0u) {
          v[k][0] = ld_tap(s00, o0 + cx0);
          v[k][1] = ld_tap(s01, o0 + cx1);
          v[k][2] = ld_tap(s10, o1 + cx0);
          v[k][3] = ld_tap(s11, o1 + cx1);
          okm |= (x + k < a.ow ? 1u : 0u) << k;
        }
      }
      // stores
      B* const orow = out + (uint64_t)y * d.row_pitch;
      const auto elem = [&](uint32_t k, uint32_t c) {
        const uint32_t sh = 8u * c, fx = (cw[k] >> RS_F_SHIFT) & 255u;
        const uint32_t acc = resize_acc((v[k][0] >> sh) & 255u, (v[k][1] >> sh) & 255u, (v[k][2] >> sh) & 255u,
                                        (v[k][3] >> sh) & 255u, fx, r.f);
        return tensor_value<DT>(resize_unit(acc), scale[c], bias[c]);
      };
      bool whole = false;
      if constexpr (P > 1) {
        whole = okm == (1u << P) - 1u;   // (no bit is set past the row's end)
        if (whole) st_group<B, P, LAYOUT>(orow, plane_pitch, x, elem);
      }
      if (!whole) {
#pragma unroll
        for (uint32_t k = 0; k < P; ++k) {
          if ((okm >> k) & 1u) st_one<B, LAYOUT>(orow, plane_pitch, x + k, [&](uint32_t c) { return elem(k, c); });
        }
      }
    }
  }
}

// Block b: band b % bands of window b / bands.
template <int DT, int LAYOUT>
__global__ __launch_bounds__(TL_THREADS) void set_resize_tensor(SetResizeArgs a) {
  const uint32_t wi = blockIdx.x / a.bands, band = blockIdx.x % a.bands;
  const SetResizeWindow d = a.wins[wi];
  const uint32_t ya = band * RS_ROWS, yb = min(ya + RS_ROWS, a.oh);
  if (d.mode == 2u) {
    set_resize_rows<DT, LAYOUT, 2>(a, d, ya, yb);
  } else if (d.mode == 1u) {
    set_resize_rows<DT, LAYOUT, 1>(a, d, ya, yb);
  } else {
    set_resize_rows<DT, LAYOUT, 0>(a, d, ya, yb);
  }
}

// (plane_pitch: 0 for an interleaved window; every group counts from output column 0)
uint32_t set_resize_window_mode(const void* d_out, uint64_t row_pitch, uint64_t plane_pitch, uint32_t dtype) {
  return vector_mode((uintptr_t)d_out, set_tensor_elem_bytes(dtype), row_pitch, plane_pitch, 0, RS_MAX_MODE);
}

int set_resize_tensor_launch(void* stream, const uint8_t* d_tiles, uint64_t tile_stride, const uint8_t* d_packed,
                             const uint64_t* d_src, const int32_t* d_slot_status, const SetResizeWindow* d_wins,
                             uint32_t n_wins, uint32_t tile_w, uint32_t tile_h, uint32_t out_w, uint32_t out_h,
                             uint32_t dtype, uint32_t layout, const float* scale, const float* bias) {
  if (n_wins == 0) return NICE_OK;
  SetResizeArgs a{d_tiles, tile_stride, d_packed, (const unsigned long long*)d_src, d_slot_status, d_wins,
                  tile_w, tile_h, out_w, out_h, (out_h + RS_ROWS - 1u) / RS_ROWS,
                  {scale[0], scale[1], scale[2]}, {bias[0], bias[1], bias[2]}};
  if ((uint64_t)n_wins * a.bands > 0x7FFFFFFFull) return NICE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(n_wins * a.bands), block(TL_THREADS);
  const int rc = tensor_dispatch(dtype, layout, [&](auto dt, auto lay) {
    hipLaunchKernelGGL((set_resize_tensor<decltype(dt)::value, decltype(lay)::value>), grid, block, 0, st, a);
  });
  return rc ? rc : hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

}  // namespace nice
