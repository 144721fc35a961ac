// nice_sets_resize_aa.hip -- image sets, antialiased resized tensor output
// (include/nice.h, "image sets: antialiased resized tensor output"): the
// windows of a set, each resampled to one out_h x out_w by the integer triangle
// filter of nice_resize.hpp, converted and stored as the tensor merges store.
// The filter is separable and the work per window proportional to its pixels:
//   1. set_resize_aa_weights: every reducing axis of every window gets its
//      weights once, in a table of 2 n_in entries of 16 bits.  A source pixel
//      lies under the taps of at most two output indices, consecutive ones, so
//      the weight of pixel i for output index x is entry 2 i + (x & 1): no
//      offsets, no lists, one thread per pixel.
//   2. set_resize_aa_tensor: a block is a window, a band of AA_ROWS output rows
//      and a chunk of 256 output columns, one per thread.  It walks the band's
//      source rows in ascending order.  The columns the chunk's taps span are
//      staged into LDS, a dword per pixel: the three bytes and, in byte +3,
//      whether the pixel's slot is readable (the slot lookup, dense or raw, is
//      made once per staged pixel).  A thread sums its column's taps (its
//      first AA_KEPT weights stay in registers for the whole band) to h[3]
//      and adds v * h to the accumulators of the band's rows; the row weights
//      v of a staged row, 0 for the rows it does not feed, stand in LDS too.
//      A span longer than the buffer is walked in chunks of AA_LDS_PX columns
//      (h stays in registers between them); a shorter one leaves room for
//      several source rows per barrier.  No tap count is bounded by anything.
// A non-reducing axis takes the two taps of resize_pos with weights in 1/4096,
// through the same code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nice.h"
#include "nice_internal.h"
#include "nice_resize.hpp"
#include "nice_sets_tensor.hpp"
#include "nice_slot_plan.hpp"
#include "nice_tiles.hpp"

namespace nice {

constexpr uint32_t AA_ROWS = 8;        // output rows per block
constexpr uint32_t AA_COLS = TL_THREADS;   // output columns per block, one per thread
// staged pixels per barrier: a row's span in chunks of this many columns, or as many whole rows as fit
constexpr uint32_t AA_LDS_PX = 2048;
constexpr uint32_t AA_MAX_STAGE_ROWS = TL_THREADS / AA_ROWS;   // a thread per (staged row, band row) weight
constexpr uint32_t AA_KEPT = 4;               // column weights a lane keeps in registers
constexpr uint32_t AA_IN_RANGE = 1u << 16;   // in a staged row weight: the row is under the band row's taps

struct SetResizeAaArgs {
  const uint8_t* tiles;
  uint64_t tile_stride;
  const uint8_t* packed;
  const unsigned long long* src;       // per position: kind and value (slot_position_sources)
  const int32_t* slot_status;          // non-null: a pixel of a slot of nonzero status is not readable
  const SetResizeAaWindow* wins;
  uint16_t* weights;                   // the weight tables of all windows
  uint32_t tw, th, ow, oh, bands, chunks;
  float scale[3], bias[3];
};

// ---- 1. the weight tables ----------------------------------------------------------
// Block b: pixels [256 c, 256 c + 256) of axis b % 2 (0 the columns) of window
// b / 2 / tchunks, c = b / 2 % tchunks.
__global__ __launch_bounds__(TL_THREADS) void set_resize_aa_weights(const SetResizeAaWindow* wins, uint16_t* weights,
                                                                     uint32_t ow, uint32_t oh, uint32_t tchunks) {
  const uint32_t axis = blockIdx.x & 1u, c = (blockIdx.x >> 1) % tchunks, wi = (blockIdx.x >> 1) / tchunks;
  const SetResizeAaWindow& d = wins[wi];
  const uint32_t n_in = axis ? d.rh : d.rw, n_out = axis ? oh : ow;
  const uint32_t i = c * TL_THREADS + threadIdx.x;
  if (n_out >= n_in || i >= n_in) return;
  uint16_t* const tab = weights + (axis ? d.wrow : d.wcol);
  // the output index whose cell holds the pixel's centre, and its neighbours
  const uint32_t xc = (2u * i + 1u) * n_out / (2u * n_in);
  for (uint32_t x = xc ? xc - 1u : 0u; x <= xc + 1u && x < n_out; ++x) {
    const ResizeAaRange r = resize_aa_range(x, n_in, n_out);
    if (i < r.lo || i > r.hi) continue;
    const uint64_t R = resize_aa_cum(r.hi, r.lo, x, n_in, n_out);
    tab[2u * i + (x & 1u)] = (uint16_t)resize_aa_weight(i, r.lo, R, x, n_in, n_out);
  }
}

// ---- 2. the filter -------------------------------------------------------------------
// The taps lo..hi of output index x of an axis, and f of resize_pos where the axis does not reduce.
struct AaTaps {
  uint32_t lo, hi, f;
};
__device__ __forceinline__ AaTaps aa_taps(uint32_t x, uint32_t n_in, uint32_t n_out) {
  if (n_out >= n_in) {
    const ResizePos p = resize_pos(x, n_in, n_out);
    return AaTaps{p.i0, p.i1, p.f};
  }
  const ResizeAaRange r = resize_aa_range(x, n_in, n_out);
  return AaTaps{r.lo, r.hi, 0u};
}
// the weight of tap i (lo <= i <= hi) of output index x; tab: the axis's table (reducing axes only)
__device__ __forceinline__ uint32_t aa_weight(const AaTaps& t, uint32_t i, uint32_t x, bool reducing, const uint16_t* tab) {
  if (reducing) return tab[2u * i + (x & 1u)];
  return i == t.lo ? resize_aa_w0(t.f) : resize_aa_w1(t.f);
}

struct __attribute__((aligned(4))) AaThree {
  uint32_t a, b, c;
};

// Pixel (i, j) of window d as the staged dword: bytes +0..+2, and 1 in byte +3
// where its slot is readable; 0 where not.
__device__ __forceinline__ uint32_t aa_fetch(const SetResizeAaArgs& a, const SetResizeAaWindow& d, uint32_t slot_row,
                                             uint32_t cy, uint32_t i) {
  const uint32_t xs = d.x0 + i, tx = xs / a.tw, cx = xs - tx * a.tw;
  const uint32_t p = slot_row + (tx - d.tx0);
  const SlotSource s = slot_source(a.src, a.slot_status, a.tiles, a.tile_stride, a.packed, p);
  if (s.bpp == 0u) return 0u;
  return (ld_tap(s, cy * a.tw + cx) & 0xFFFFFFu) | (1u << 24);   // (a tile has at most 2^26 pixels)
}

// Block b: chunk b % chunks of band b / chunks % bands of window b / chunks / bands.
template <int DT, int LAYOUT>
__global__ __launch_bounds__(TL_THREADS) void set_resize_aa_tensor(SetResizeAaArgs a) {
  using B = typename TensorElem<DT>::bits;
  __shared__ uint32_t px[AA_LDS_PX];
  __shared__ uint32_t vw[TL_THREADS];   // [staged row][band row]: the weight, AA_IN_RANGE where the row is under its taps
  const uint32_t chunk = blockIdx.x % a.chunks, band = blockIdx.x / a.chunks % a.bands, wi = blockIdx.x / a.chunks / a.bands;
  const SetResizeAaWindow d = a.wins[wi];
  const uint32_t tid = threadIdx.x;
  const uint32_t ya = band * AA_ROWS, yb = min(ya + AA_ROWS, a.oh);
  const uint32_t xa = chunk * AA_COLS, xb = min(xa + AA_COLS, a.ow);
  const bool red_x = a.ow < d.rw, red_y = a.oh < d.rh;
  // (addresses the lanes add to: kept out of the scalar registers)
  const uint16_t* const wcol = a.weights + in_vgpr(d.wcol);
  const uint16_t* const wrow = a.weights + in_vgpr(d.wrow);
  // the block's source rows and columns (everything here is the same in every lane)
  const uint32_t jlo = aa_taps(ya, d.rh, a.oh).lo, jhi = aa_taps(yb - 1u, d.rh, a.oh).hi;
  const AaTaps ca = aa_taps(d.flip ? a.ow - 1u - xa : xa, d.rw, a.ow);
  const AaTaps cb = aa_taps(d.flip ? a.ow - 1u - (xb - 1u) : xb - 1u, d.rw, a.ow);
  const uint32_t slo = min(ca.lo, cb.lo), shi = max(ca.hi, cb.hi), span = shi - slo + 1u;
  const uint32_t cw = min(span, AA_LDS_PX);                              // columns per stage
  const uint32_t nr = min(AA_LDS_PX / cw, AA_MAX_STAGE_ROWS);            // rows per stage: 1 where the span is chunked
  // the lane's column
  const uint32_t x = xa + tid;
  const bool active = x < xb;
  const uint32_t xs = d.flip ? a.ow - 1u - x : x;
  AaTaps t = aa_taps(active ? xs : 0u, d.rw, a.ow);
  if (!active) t.hi = 0u, t.lo = 1u;   // no taps
  // its first AA_KEPT weights, the same for every source row, stay in registers; longer runs read the rest from the table
  uint32_t wk[AA_KEPT];
#pragma unroll
  for (uint32_t k = 0; k < AA_KEPT; ++k) wk[k] = (active && t.lo + k <= t.hi) ? aa_weight(t, t.lo + k, xs, red_x, wcol) : 0u;
  uint32_t acc[AA_ROWS][3], h[3] = {0u, 0u, 0u};
  uint32_t hok = 1u, bad = 0u;   // bad, bit y: an unreadable pixel under band row y's taps
#pragma unroll
  for (uint32_t y = 0; y < AA_ROWS; ++y) acc[y][0] = acc[y][1] = acc[y][2] = 0u;

  for (uint32_t j0 = jlo; j0 <= jhi; j0 += nr) {
    const uint32_t rows = min(nr, jhi - j0 + 1u);
    for (uint32_t c0 = slo; c0 <= shi; c0 += cw) {
      const uint32_t cols = min(cw, shi - c0 + 1u);
      __syncthreads();   // the stage before is read
      // (staged rows and columns flattened over the threads: a narrow span keeps the block busy)
      for (uint32_t k = tid; k < rows * cols; k += TL_THREADS) {
        const uint32_t r = k / cols, c = k - r * cols;
        const uint32_t ys = d.y0 + j0 + r, ty = ys / a.th, cy = ys - ty * a.th;
        px[k] = aa_fetch(a, d, d.slot_first + (ty - d.ty0) * d.ntx, cy, c0 + c);
      }
      if (c0 == slo && tid < rows * AA_ROWS) {
        const uint32_t r = tid / AA_ROWS, y = ya + tid % AA_ROWS, j = j0 + r;
        uint32_t w = 0u;
        if (y < yb) {
          const AaTaps rt = aa_taps(y, d.rh, a.oh);
          if (j >= rt.lo && j <= rt.hi) w = aa_weight(rt, j, y, red_y, wrow) | AA_IN_RANGE;
        }
        vw[tid] = w;
      }
      __syncthreads();
      const uint32_t i0 = max(t.lo, c0), i1 = min(t.hi, c0 + cols - 1u);   // the lane's taps in this stage (none: i0 > i1)
      const bool last = c0 + cols > shi;
      for (uint32_t r = 0; r < rows; ++r) {
        for (uint32_t i = i0; i <= i1; ++i) {
          const uint32_t p = px[r * cols + (i - c0)], k = i - t.lo;
          const uint32_t w = k == 0u ? wk[0] : k == 1u ? wk[1] : k == 2u ? wk[2] : k == 3u ? wk[3] : aa_weight(t, i, xs, red_x, wcol);
          h[0] += w * (p & 255u);
          h[1] += w * ((p >> 8) & 255u);
          h[2] += w * ((p >> 16) & 255u);
          hok &= p >> 24;
        }
        if (last) {   // the row's h is whole
#pragma unroll
          for (uint32_t y = 0; y < AA_ROWS; ++y) {
            const uint32_t v = vw[r * AA_ROWS + y];
            acc[y][0] += (v & 0xFFFFu) * h[0];
            acc[y][1] += (v & 0xFFFFu) * h[1];
            acc[y][2] += (v & 0xFFFFu) * h[2];
            bad |= ((v >> 16) & (hok ^ 1u)) << y;
          }
          h[0] = h[1] = h[2] = 0u;
          hok = 1u;
        }
      }
    }
  }
  if (!active) return;
  B* const out = reinterpret_cast<B*>(d.out);
  const uint64_t row_pitch = in_vgpr64(d.row_pitch), plane_pitch = in_vgpr64(d.plane_pitch);
#pragma unroll
  for (uint32_t y = 0; y < AA_ROWS; ++y) {
    if (ya + y < yb && !((bad >> y) & 1u)) {
      B* const orow = out + (uint64_t)(ya + y) * row_pitch;
      B e[3];
#pragma unroll
      for (uint32_t c = 0; c < 3; ++c)
        e[c] = tensor_value<DT>(resize_unit(resize_aa_round(acc[y][c])), a.scale[c], a.bias[c]);
      if constexpr (LAYOUT == (int)NICE_TENSOR_INTERLEAVED && sizeof(B) == 4) {
        // a pixel's three float32 are 12 bytes at 4-byte alignment: one store
        *reinterpret_cast<AaThree*>(orow + 3ull * x) = AaThree{e[0], e[1], e[2]};
      } else {
        st_one<B, LAYOUT>(orow, plane_pitch, x, [&](uint32_t c) { return e[c]; });
      }
    }
  }
}

uint64_t set_resize_aa_table_entries(uint32_t n_in, uint32_t n_out) { return n_out < n_in ? 2ull * n_in : 0ull; }

int set_resize_aa_tensor_launch(void* stream, const uint8_t* d_tiles, uint64_t tile_stride, const uint8_t* d_packed,
                                const uint64_t* d_src, const int32_t* d_slot_status, const SetResizeAaWindow* d_wins,
                                uint32_t n_wins, uint16_t* d_weights, uint32_t max_reducing, uint32_t tile_w,
                                uint32_t tile_h, uint32_t out_w, uint32_t out_h, uint32_t dtype, uint32_t layout,
                                const float* scale, const float* bias) {
  if (n_wins == 0) return NICE_OK;
  SetResizeAaArgs a{d_tiles, tile_stride, d_packed, (const unsigned long long*)d_src, d_slot_status, d_wins, d_weights,
                    tile_w, tile_h, out_w, out_h, (out_h + AA_ROWS - 1u) / AA_ROWS, (out_w + AA_COLS - 1u) / AA_COLS,
                    {scale[0], scale[1], scale[2]}, {bias[0], bias[1], bias[2]}};
  const uint32_t tchunks = max_reducing ? (max_reducing + TL_THREADS - 1u) / TL_THREADS : 1u;
  if (2ull * n_wins * tchunks > 0x7FFFFFFFull || (uint64_t)n_wins * a.bands * a.chunks > 0x7FFFFFFFull) return NICE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(n_wins * a.bands * a.chunks), block(TL_THREADS);
  const int rc = tensor_dispatch(dtype, layout, [&](auto dt, auto lay) {   // (an unknown dtype launches neither)
    hipLaunchKernelGGL(set_resize_aa_weights, dim3(2u * n_wins * tchunks), block, 0, st, d_wins, d_weights, out_w, out_h,
                       tchunks);
    hipLaunchKernelGGL((set_resize_aa_tensor<decltype(dt)::value, decltype(lay)::value>), grid, block, 0, st, a);
  });
  return rc ? rc : hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

}  // namespace nice
