// nice_classify.hip -- MI355X (gfx950) classify pass of the NICE2 encoder: the
// first kernel of nice_encode.hip's pipeline.  Per pixel the mode decision
// (code.rs:159-369) and its record, per frame the symbol histogram
// (hfe.rs:29-45), per tile the first / last coded pixel.
//   enc_classify, _tiny      tiles staged as 4 row windows (any stride, W < 3)
//   enc_classify_ring*       a block walks its tiles keeping an LDS ring of pixels
//   enc_classify_pair*       the ring with two tiles per iteration
//   enc_classify_slide0..3   per-lane sliding windows (the bench path)
//   enc_classify_strip*      vertical strips of rows too wide for a ring
//   enc_classify_twin*       per-tile row windows for every other wide shape
//   enc_rundigits            run digits from the coded flags the _m forms and
//                            the slide kernel write
// The ring, pair, slide, strip and twin bodies differ in how they stage
// pixels; the stages they share are the cls_* functions below, the per-pixel
// decision is classify_y / classify_win and its arithmetic nice_classify.hpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nice_classify.hpp"
#include "nice_enc_shared.hpp"
#include "nice_format.h"
#include "nice_kernels.h"
#include "nice_rec.hpp"

namespace nice {

// (ENC_TILE, ENC_THREADS and every other block size: nice_geom.h)
constexpr int PX_PER_THREAD = ENC_TILE / ENC_THREADS;  // 4
constexpr int WIN = ENC_TILE + 6;

// ---------------------------------------------------------------------------
// Tile staging: 4 windows, window k holds X' of pixels [start - kW - 3, start - kW - 3 + WIN).
// Out-of-frame positions hold 0 and are never used (classify<false> checks validity).
// ---------------------------------------------------------------------------
struct TileWin {
  uint32_t w[4][WIN];
};

__device__ __forceinline__ uint32_t load_spread(const uint8_t* __restrict__ frame, int64_t j, int C) {
  if (C == 4) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(frame + j * 4);
    return spread_rgba(v);
  }
  const uint8_t* p = frame + j * C;
  return spread_rgb(p[0], p[1], p[2]);
}

__device__ inline void stage_tile(TileWin& tw, const uint8_t* __restrict__ frame, int64_t start,
                                  int64_t lo, int64_t hi, uint32_t W, int C) {
  for (int k = 0; k < 4; ++k) {
    const int64_t base = start - (int64_t)k * W - 3;
    for (int j = threadIdx.x; j < WIN; j += ENC_THREADS) {
      const int64_t g = base + j;
      tw.w[k][j] = (g >= lo && g < hi) ? load_spread(frame, g, C) : 0u;
    }
  }
}

// Software-pipelined staging for 4-byte pixels: raw words of the next tile are
// loaded into registers while the current tile is classified, then spread
// into the LDS windows.
constexpr int STAGE_PER_THREAD = (WIN + ENC_THREADS - 1) / ENC_THREADS;   // 5
struct TilePrefetch {
  uint32_t v[4][STAGE_PER_THREAD];
};
__device__ __forceinline__ void prefetch_tile(TilePrefetch& pf, const uint8_t* __restrict__ frame,
                                              int64_t start, int64_t lo, int64_t hi, uint32_t W) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t base = start - (int64_t)k * W - 3;
#pragma unroll
    for (int i = 0; i < STAGE_PER_THREAD; ++i) {
      const int j = (int)threadIdx.x + i * ENC_THREADS;
      const int64_t g = base + j;
      pf.v[k][i] = (j < WIN && g >= lo && g < hi) ? reinterpret_cast<const uint32_t*>(frame)[g] : 0u;
    }
  }
}
__device__ __forceinline__ void commit_tile(TileWin& tw, const TilePrefetch& pf) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int i = 0; i < STAGE_PER_THREAD; ++i) {
      const int j = (int)threadIdx.x + i * ENC_THREADS;
      if (j < WIN) tw.w[k][j] = spread_rgba(pf.v[k][i]);
    }
  }
}

struct WinAcc {
  const TileWin* tw;
  int col;  // p + 3
  __device__ __forceinline__ uint32_t operator()(int rows, int px) const { return tw->w[rows][col - px]; }
};

// ---------------------------------------------------------------------------
// K1: classify + histogram + per-pixel symbol records.
//
// Record (one u32 per pixel, raster order): bits 0..2 the mode prefix
// (P_BACK_REF .. P_LUMA2) or REC_UNCODED for a run member; bits 3.. the payload,
// laid out as the classify arithmetic produces it (the spread/luma-space
// fields at 10-bit spacing, masked and shifted once):
//   BACK_REF  k (3) at 3            SMALL_DIFF  index 0..342 (9) at 3
//   LUMA2     r+16 (5) at 3, g+32 (6) at 13, b+16 (5) at 23
//   LUMA      k (4) at 3, r+16 (5) at 7, g+32 (6) at 17, b+16 (5) at 27
//   RGB       r, g, b residuals (8 each) at 3, 13, 23
// ---------------------------------------------------------------------------
constexpr uint32_t REC_UNCODED = 7u;
// the luma payload fields of Y(X) - Y(ref) (r: bits 0-4, g: 10-15, b: 20-24)
constexpr uint32_t LUMA_FIELDS = 0x1Fu | (0x3Fu << 10) | (0x1Fu << 20);

__device__ __forceinline__ uint32_t rec_from_syms(const PixSyms& s) {
  switch (s.mode) {
    case P_BACK_REF: return P_BACK_REF | ((s.b[0] - BIN_BACK_REF) << 3);
    case P_SMALL_DIFF: return P_SMALL_DIFF | ((s.b[0] - BIN_SMALL_DIFF) << 3);
    case P_LUMA2:
      return P_LUMA2 | ((s.b[0] - BIN_LUMA2_BASE) << 13) | ((s.b[1] - BIN_LUMA2_R) << 3) |
             ((s.b[2] - BIN_LUMA2_B) << 23);
    case P_LUMA:
      return P_LUMA | ((s.b[0] - BIN_LUMA_REF) << 3) | ((s.b[1] - BIN_LUMA_BASE) << 17) |
             ((s.b[2] - BIN_LUMA_OTHER) << 7) | ((s.b[3] - BIN_LUMA_OTHER) << 27);
    default: return P_RGB | (s.b[0] << 3) | (s.b[1] << 13) | (s.b[2] << 23);
  }
}

// Payload bins of a coded record (n = 1, 3 or 4), branch-free: per mode m
// (record bits 0..2), payload k is bits [shift, shift+width) of the record plus
// a histogram base, all looked up in packed constants (no per-mode control flow).
//   m:        0 BACK_REF   1 RGB        2 LUMA        3 SMALL_DIFF  4 LUMA2
//   k = 0     847+[3,3)    0+[3,8)      365+[3,4)     376+[3,9)     719+[13,6)
//   k = 1     -            0+[13,8)     269+[17,6)    -             783+[3,5)
//   k = 2     -            0+[23,8)     333+[7,5)     -             815+[23,5)
//   k = 3     -            -            333+[27,5)    -             -
constexpr unsigned long long rb_pack(int a0, int a1, int a2, int a3, int a4, int bits) {
  return (unsigned long long)a0 | ((unsigned long long)a1 << bits) | ((unsigned long long)a2 << (2 * bits)) |
         ((unsigned long long)a3 << (3 * bits)) | ((unsigned long long)a4 << (4 * bits));
}
// base (10 bits per mode), shift (5) | width << 5 (10 bits per mode)
constexpr unsigned long long RB_BASE[4] = {
    rb_pack(BIN_BACK_REF, 0, BIN_LUMA_REF, BIN_SMALL_DIFF, BIN_LUMA2_BASE, 10),
    rb_pack(0, 0, BIN_LUMA_BASE, 0, BIN_LUMA2_R, 10),
    rb_pack(0, 0, BIN_LUMA_OTHER, 0, BIN_LUMA2_B, 10),
    rb_pack(0, 0, BIN_LUMA_OTHER, 0, 0, 10)};
constexpr unsigned long long RB_FIELD[4] = {
    rb_pack(3 | 3 << 5, 3 | 8 << 5, 3 | 4 << 5, 3 | 9 << 5, 13 | 6 << 5, 10),
    rb_pack(0, 13 | 8 << 5, 17 | 6 << 5, 0, 3 | 5 << 5, 10),
    rb_pack(0, 23 | 8 << 5, 7 | 5 << 5, 0, 23 | 5 << 5, 10),
    rb_pack(0, 0, 27 | 5 << 5, 0, 0, 10)};
constexpr uint32_t RB_N = 1u | 3u << 3 | 4u << 6 | 1u << 9 | 3u << 12;   // payload count, 3 bits per mode
__device__ __forceinline__ uint32_t rb_bin(uint32_t rec, uint32_t m, int k) {
  const uint32_t base = (uint32_t)(RB_BASE[k] >> (10u * m)) & 0x3FFu;
  const uint32_t fw = (uint32_t)(RB_FIELD[k] >> (10u * m)) & 0x3FFu;
  return base + __builtin_amdgcn_ubfe(rec, fw & 31u, fw >> 5);
}
__device__ __forceinline__ uint32_t rec_bins(uint32_t rec, uint32_t& b0, uint32_t& b1, uint32_t& b2,
                                             uint32_t& b3) {
  const uint32_t m = min(rec & 7u, 4u);
  b0 = rb_bin(rec, m, 0);
  b1 = rb_bin(rec, m, 1);
  b2 = rb_bin(rec, m, 2);
  b3 = rb_bin(rec, m, 3);
  return (RB_N >> (3u * m)) & 7u;
}
// Window-classify record (layout above) -> the packer's record (nice_rec.hpp).
__device__ __forceinline__ uint32_t rec2_from_old(uint32_t rec, uint32_t lane) {
  const uint32_t m = rec & 7u;
  if (m == REC_UNCODED) return rec2_unc(lane);
  if (m == P_BACK_REF) return ((C0_BR + ((rec >> 3) & 7u)) << 3) | rec2_abs(lane);
  if (m == P_SMALL_DIFF) return ((C0_SD + ((rec >> 3) & 0x1FFu)) << 3) | rec2_abs(lane);
  if (m == P_LUMA2)
    return ((C0_L2 + ((rec >> 13) & 0x3Fu)) << 3) | ((SX_L2 + ((rec >> 3) & 0x1Fu)) << 14) |
           ((SX_L2 + ((rec >> 23) & 0x1Fu)) << 23);
  if (m == P_LUMA)
    return ((C0_LUMA + 64u * ((rec >> 3) & 15u) + ((rec >> 17) & 0x3Fu)) << 3) |
           ((SX_LUMA + ((rec >> 7) & 0x1Fu)) << 14) | ((SX_LUMA + ((rec >> 27) & 0x1Fu)) << 23);
  return (((rec >> 3) & 0xFFu) << 3) | (((rec >> 13) & 0xFFu) << 14) | (((rec >> 23) & 0xFFu) << 23);
}

// Branch-free mode decision from the LDS windows (column col = p + 3 of window
// `rows`, pixel i - (rows*W + px) at col - px): all tests are evaluated and the
// first hit in the reference order wins (code.rs:191-366).  HEAD = false: every
// reference exists (i >= 3W+3, W >= 3).  HEAD = true (W >= 3): the reference's
// validity rules as masks, as in classify_ring<true>.
template <bool HEAD>
__device__ __forceinline__ uint32_t classify_fast(const TileWin& tw, int col, uint32_t i, uint32_t W) {
  const uint32_t X = tw.w[0][col], L2 = tw.w[0][col - 2], L3 = tw.w[0][col - 3];
  uint32_t L = tw.w[0][col - 1];
  const uint32_t U = tw.w[1][col], UR1 = tw.w[1][col + 1], UR3 = tw.w[1][col + 3], UL3 = tw.w[1][col - 3];
  const uint32_t U2 = tw.w[2][col];
  const uint32_t V = tw.w[3][col], VR1 = tw.w[3][col + 1], VL1 = tw.w[3][col - 1];
  const uint32_t VL3 = tw.w[3][col - 3], VR3 = tw.w[3][col + 3];
  // back references k = 1..4 (k = 0, the pixel before, never equals a coded pixel)
  bool e1 = U == X, e2 = UR1 == X, e3 = L2 == X, e4 = U2 == X;
  const bool has_up = !HEAD || i >= W, has_left = !HEAD || i > 0;
  if constexpr (HEAD) {
    e1 = e1 && i >= W;
    e2 = e2 && i >= W - 1u;
    e3 = e3 && i >= 2u;
    e4 = e4 && i >= 2u * W;
    L = i > 0 ? L : X;
  }
  const bool br = e1 | e2 | e3 | e4;
  const uint32_t bk = e1 ? 1u : e2 ? 2u : e3 ? 3u : 4u;
  const uint32_t pred = has_up ? avg3(U, L) : L;
  // small diff
  const uint32_t d = X + K3(259u) - pred;
  const bool sd = has_left && ((d & K3(0x3F8u)) == K3(0x100u)) && ((((d & K3(7u)) + K3(1u)) & K3(8u)) == 0);
  const uint32_t sdi = (d & 7u) + 7u * ((d >> 10) & 7u) + 49u * ((d >> 20) & 7u);
  // luma2 against the average
  const uint32_t xk = X + LUMA_K;
  const uint32_t t2 = luma_t(xk, pred);
  const bool l2 = has_up && (t2 & LUMA_MASK) == 0;
  // luma against 11 references, first hit wins; skipped when no lane needs it
  uint32_t lk = 11u, lt = 0u;
  const bool need_luma = __builtin_amdgcn_ballot_w64(!br && !sd && !l2) != 0ull;
  if (need_luma) {
    const uint32_t refs[11] = {L, U, UR1, UR3, L3, VR1, V, VL1, UL3, VL3, VR3};
#pragma unroll
    for (int k = 10; k >= 0; --k) {
      const uint32_t t = luma_t(xk, refs[k]);
      bool ok = (t & LUMA_MASK) == 0;
      if constexpr (HEAD) ok = ok && i > 0 && i >= (uint32_t)lr_rows(k) * W + (uint32_t)lr_px(k);
      lk = ok ? (uint32_t)k : lk;
      lt = ok ? t : lt;
    }
  }
  const uint32_t r = X + K3(256u) - (has_left ? pred : 0u);
  const uint32_t rec_br = P_BACK_REF | (bk << 3);
  const uint32_t rec_sd = P_SMALL_DIFF | (sdi << 3);
  const uint32_t rec_l2 = P_LUMA2 | ((t2 & LUMA_FIELDS) << 3);
  const uint32_t rec_lu = P_LUMA | (lk << 3) | ((lt & LUMA_FIELDS) << 7);
  const uint32_t rec_rgb = P_RGB | ((r & K3(0xFFu)) << 3);
  return br ? rec_br : sd ? rec_sd : l2 ? rec_l2 : lk < 11u ? rec_lu : rec_rgb;
}

// TINY (W < 3): references wrap inside the window rows; the general
// classify<false> decides the first 3W+3 pixels (all of a tiny frame).
template <bool TINY>
__device__ __forceinline__ void enc_classify_body(const EncArgs& a) {
  __shared__ TileWin tw;
  __shared__ uint32_t hist[N_BINS];
  __shared__ uint32_t mask[ENC_TILE / 32];

  // work items: frame f, band tile tt in [tile_lo, tile_hi); t = f*T + tt
  const uint32_t nt = a.tile_hi - a.tile_lo;
  const uint64_t total_work = (uint64_t)a.n_frames * nt;
  const uint64_t w_begin = (uint64_t)blockIdx.x * a.tiles_per_block;
  uint64_t w_end = w_begin + a.tiles_per_block;
  if (w_end > total_work) w_end = total_work;
  if (w_begin >= w_end) return;

  for (int b = threadIdx.x; b < N_BINS; b += ENC_THREADS) hist[b] = 0;
  uint32_t cur_frame = (uint32_t)(w_begin / nt);
  const int lane = threadIdx.x & 63;
  const int64_t N = (int64_t)a.W * a.H;
  const bool rgba = a.C == 4;
  TilePrefetch pf;
  if (rgba) {
    const uint32_t f0 = (uint32_t)(w_begin / nt);
    prefetch_tile(pf, a.px + (uint64_t)f0 * a.frame_stride,
                  (int64_t)(a.tile_lo + w_begin % nt) * ENC_TILE, a.px_lo, a.px_hi, a.W);
  }

  for (uint64_t w = w_begin; w < w_end; ++w) {
    const uint32_t f = (uint32_t)(w / nt);
    const uint32_t tt = a.tile_lo + (uint32_t)(w % nt);
    const uint64_t t = (uint64_t)f * a.tiles_per_frame + tt;
    if (f != cur_frame) {
      __syncthreads();
      for (int b = threadIdx.x; b < N_BINS; b += ENC_THREADS) {
        if (hist[b]) atomicAdd(&a.hist[(uint64_t)cur_frame * N_BINS + b], hist[b]);
        hist[b] = 0;
      }
      cur_frame = f;
    }
    const uint8_t* frame = a.px + (uint64_t)f * a.frame_stride;
    const int64_t start = (int64_t)tt * ENC_TILE;
    const int count = (int)((N - start) < ENC_TILE ? (N - start) : ENC_TILE);
    __syncthreads();
    if (rgba) {
      commit_tile(tw, pf);
      if (w + 1 < w_end) {   // next tile's pixels are in flight while this one is classified
        const uint32_t f1 = (uint32_t)((w + 1) / nt);
        prefetch_tile(pf, a.px + (uint64_t)f1 * a.frame_stride,
                      (int64_t)(a.tile_lo + (w + 1) % nt) * ENC_TILE, a.px_lo, a.px_hi, a.W);
      }
    } else {
      stage_tile(tw, frame, start, a.px_lo, a.px_hi, a.W, a.C);
    }
    __syncthreads();

    // coded flags -> bitmask
    uint32_t coded_bits = 0;
#pragma unroll
    for (int r = 0; r < PX_PER_THREAD; ++r) {
      const int p = r * ENC_THREADS + threadIdx.x;
      const int64_t i = start + p;
      bool coded = false;
      if (p < count) coded = (i == 0) || (tw.w[0][p + 3] != tw.w[0][p + 2]);
      const unsigned long long bal = __ballot(coded);
      if (lane == 0) {
        const int wbase = (r * ENC_THREADS + (threadIdx.x & ~63)) >> 5;
        mask[wbase] = (uint32_t)bal;
        mask[wbase + 1] = (uint32_t)(bal >> 32);
      }
      coded_bits |= (coded ? 1u : 0u) << r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int first = -1, last = -1;
      for (int w = 0; w < ENC_TILE / 32; ++w)
        if (mask[w]) { first = w * 32 + __builtin_ctz(mask[w]); break; }
      for (int w = ENC_TILE / 32 - 1; w >= 0; --w)
        if (mask[w]) { last = w * 32 + 31 - __builtin_clz(mask[w]); break; }
      a.tile_first[t] = first < 0 ? NONE : (uint32_t)(start + first);
      a.tile_last[t] = last < 0 ? NONE : (uint32_t)(start + last);
    }
    const bool fast = (a.W >= 3) && (start >= 3 * (int64_t)a.W + 3);
    uint32_t* recs = a.recs + (uint64_t)f * a.rec_stride + start;
#pragma unroll
    for (int r = 0; r < PX_PER_THREAD; ++r) {
      const int p = r * ENC_THREADS + threadIdx.x;
      const bool coded = (coded_bits >> r) & 1u;
      uint32_t rec = REC_UNCODED;
      if (fast) {
        const uint32_t rf = classify_fast<false>(tw, p + 3, 0u, a.W);
        rec = coded ? rf : REC_UNCODED;
      } else if constexpr (TINY) {
        if (coded) {
          PixSyms s;
          WinAcc acc{&tw, p + 3};
          classify<false>((uint32_t)(start + p), a.W, acc, s);
          rec = rec_from_syms(s);
        }
      } else {   // block-uniform branch: both variants are straight-line code
        const uint32_t rf = classify_fast<true>(tw, p + 3, (uint32_t)(start + p), a.W);
        rec = coded ? rf : REC_UNCODED;
      }
      if (p < count) recs[p] = rec2_from_old(rec, (uint32_t)lane);
      if (coded) {
        uint32_t b0, b1, b2, b3;
        const uint32_t n = rec_bins(rec, b0, b1, b2, b3);
        atomicAdd(&hist[b0], 1u);
        if (n > 1) { atomicAdd(&hist[b1], 1u); atomicAdd(&hist[b2], 1u); }
        if (n > 3) atomicAdd(&hist[b3], 1u);
        const int nx = next_coded_local(mask, p);
        if (nx < count) {
          const uint64_t run = (uint64_t)(nx - p - 1);
          if (run > 0) {
            uint64_t m = run - 1;
            while (true) {
              atomicAdd(&hist[BIN_PREFIX + P_RUN1 + (uint32_t)(m & 7u)], 1u);
              if (m < 8) break;
              m >>= 3;
            }
          }
        }
      }
      // mode prefixes: derived by enc_tables from the payload streams (mode_id_bin)
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < N_BINS; b += ENC_THREADS)
    if (hist[b]) atomicAdd(&a.hist[(uint64_t)cur_frame * N_BINS + b], hist[b]);
}
__global__ __launch_bounds__(ENC_THREADS) void enc_classify(EncArgs a) { enc_classify_body<false>(a); }
__global__ __launch_bounds__(ENC_THREADS) void enc_classify_tiny(EncArgs a) { enc_classify_body<true>(a); }

// ---------------------------------------------------------------------------
// K1r: classify, ring-staged (RGBA frames, 3 <= W <= CLS_RING_MAX_W).
//
// Same outputs as enc_classify (records, histogram, tile first/last coded
// pixel), restructured for the instruction budget:
//  * every pixel is loaded from HBM and converted once: a block walks its tile
//    range in raster order and keeps the last CLS_RING pixels (>= 3 rows + 3 px
//    + one tile) in an LDS ring indexed by pixel & (CLS_RING - 1); the next
//    tile is loaded into registers while the current one is classified;
//  * pixels are held in "luma space", Y = (R-G) | G << 10 | (B-G) << 20 (each
//    field mod 256).  The transform is a bijection, so the equality tests of
//    back references and runs hold unchanged, and the luma test of code.rs:
//    296-336 against reference pixel R -- g = XG-RG in [-32,32), XR-RR-g and
//    XB-RB-g in [-16,16) -- becomes a range test on the field-wise difference
//    Y(X) - Y(R): one subtract, one AND, one compare per reference;
//  * the five mode-prefix counts are accumulated per thread in packed
//    registers and added to the histogram once per frame.
// ---------------------------------------------------------------------------
// (CLS_THREADS, CLS_RING: nice_geom.h)
constexpr int CLS_PPT = ENC_TILE / CLS_THREADS;   // 2 pixels per thread
// words 0..CLS_GUARD-1 of the ring mirrored past its end: a neighbour group
// (pixels b .. b+6 for b = ((s - rows*W - 3) mod CLS_RING) + tid, s the
// wave-uniform part of the pixel index) is one base address plus immediate
// offsets, never wrapping
constexpr int CLS_GUARD = CLS_THREADS + 8;
// luma test offsets in Y space: R,B fields +16, G field +32, plus 256 per field
constexpr uint32_t LUMA_KY = (256u + 16u) | ((256u + 32u) << 10) | ((256u + 16u) << 20);

// (R-G, B-G) by one packed 16-bit subtract of G from the halves G<<8|R and
// A<<8|B (borrows land in the G and A bytes, masked off), then B-G moved up by
// one 24-bit multiply-add: 7 VALU instead of 11 for the spread-and-subtract
// form (both checked equal over every RGB value on the host)
typedef unsigned short nice_u16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int nice_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t y_from_rgba(uint32_t v) {
  const uint32_t g = __builtin_amdgcn_ubfe(v, 8, 8);
  const nice_u16x2 d = __builtin_bit_cast(nice_u16x2, v) - __builtin_bit_cast(nice_u16x2, g | (g << 16));
  const uint32_t t = __builtin_bit_cast(uint32_t, d);
  return (__umul24(t & 0xFF0000u, 16u) + (t & 0xFFu)) | (g << 10);
}
__device__ __forceinline__ uint32_t rgb_from_y(uint32_t y) {
  // g | g << 20 as one 24-bit multiply-add (v_bfe + v_mad_u32_u24 + v_and)
  const uint32_t g = (y >> 10) & 0xFFu;
  return (y + __umul24(g, 0x100001u)) & K3(0xFFu);
}

// Branch-free mode decision from the Y ring; returns the record (same layout
// as classify_fast).  Four base addresses (rows 0..3 back, 3 pixels left), the
// rest immediate offsets: for pixel i = s + tid (s wave-uniform) base k is
// ring + ((s - c_k) mod RING) + tid, a scalar plus the thread index (the
// mirrored guard covers the overrun past the ring's end).
// HEAD = false: every reference valid (i >= 3W+3, W >= 3).  HEAD = true: the
// first tiles of a frame, with the reference's validity rules as masks instead
// of classify<false>'s early exits (code.rs:191-366; W >= 3): a reference
// counts only if i >= its offset, L is X itself at i = 0, without a row above
// the prediction is L and LUMA2 is skipped, SMALL_DIFF and LUMA need i > 0, and
// the raw residual is taken against 0 at i = 0.  (The back reference to pixel
// i-1 can never hit a coded pixel, so it is not tested.)
// The four neighbour groups of the lane's pixel: b0 = pixels i-3 .. i (row y),
// b1 = row y-1 from 3 left, b2 = pixel i-2W, b3 = row y-3 from 3 left; the
// hit's difference is read again at rbase[ltab[k] + tid].
// X: the lane's own pixel (Y space), from the caller's registers where it
// staged it (saves one ring read per pixel).
template <bool HEAD>
__device__ __forceinline__ uint32_t classify_y(const uint32_t* b0, const uint32_t* b1, const uint32_t* b2,
                                               const uint32_t* b3, const uint32_t* rbase, uint32_t tid, uint32_t W,
                                               uint32_t i, const uint32_t* ltab, uint32_t cbr, uint32_t csd,
                                               uint32_t X);
template <bool HEAD, int RING = CLS_RING>
__device__ __forceinline__ uint32_t classify_ring(const uint32_t* ring, uint32_t s, uint32_t tid, uint32_t W,
                                                  uint32_t i, const uint32_t* ltab, uint32_t cbr, uint32_t csd,
                                                  uint32_t X) {
  return classify_y<HEAD>(ring + ((s - 3u) & (RING - 1)) + tid, ring + ((s - W - 3u) & (RING - 1)) + tid,
                          ring + ((s - 2u * W) & (RING - 1)) + tid,
                          ring + ((s - 3u * W - 3u) & (RING - 1)) + tid, ring, tid, W, i, ltab, cbr, csd, X);
}
template <bool HEAD>
__device__ __forceinline__ uint32_t classify_y(const uint32_t* b0, const uint32_t* b1, const uint32_t* b2,
                                               const uint32_t* b3, const uint32_t* rbase, uint32_t tid, uint32_t W,
                                               uint32_t i, const uint32_t* ltab, uint32_t cbr, uint32_t csd,
                                               uint32_t X) {
  const uint32_t L2 = b0[1], L3 = b0[0];
  uint32_t L = b0[2];
  const uint32_t U = b1[3], UR1 = b1[4], UR3 = b1[6], UL3 = b1[0];
  const uint32_t U2 = b2[0];
  const uint32_t V = b3[3], VR1 = b3[4], VL1 = b3[2];
  const uint32_t VL3 = b3[0], VR3 = b3[6];
  // back references k = 1..4 (code.rs:191-206; Y equality == RGB equality)
  bool e1 = U == X, e2 = UR1 == X, e3 = L2 == X, e4 = U2 == X;
  const bool has_up = !HEAD || i >= W, has_left = !HEAD || i > 0;
  if constexpr (HEAD) {
    e1 = e1 && i >= W;
    e2 = e2 && i >= W - 1u;
    e3 = e3 && i >= 2u;
    e4 = e4 && i >= 2u * W;
    L = i > 0 ? L : X;
  }
  const bool br = e1 | e2 | e3 | e4;
  const uint32_t bk = e1 ? 1u : e2 ? 2u : e3 ? 3u : 4u;
  // prediction floor((U+L)/2) in RGB (L alone without a row above)
  const uint32_t xr = rgb_from_y(X);
  const uint32_t lrgb = rgb_from_y(L);
  const uint32_t pred = has_up ? avg3(rgb_from_y(U), lrgb) : lrgb;
  // small diff (code.rs:208-247)
  const uint32_t d = xr + K3(259u) - pred;
  // every field in [256, 262]: bits 3-9 0b0100000 (field in [256, 263]) and
  // bit 3 of field + 1 clear (field != 263), OR-ed so one compare covers all
  // three fields (an OR only adds bit 3, which 0x100 lacks; no carry: fields
  // <= 515)
  const bool sd = has_left && ((d & K3(0x3F8u)) | ((d + K3(1u)) & K3(8u))) == K3(0x100u);
  // the index f0 + 7 f1 + 49 f2 of the three 3-bit fields f (code.rs:243-245)
  // by one 24-bit multiply: the product's bits 20..29 hold it, the partial
  // products below stay under 2^20 (f <= 6) and the ones above start at bit 30
  const uint32_t sdi = (__umul24(d & K3(7u), 49u | (7u << 10) | (1u << 20)) >> 20) & 0x3FFu;
  // luma2 against the prediction (code.rs:252-292): t2 = Y(X) - Y(pred) with
  // the test offsets, Y(pred) = pred - pg in fields 0 and 2, written as
  // X + LUMA_KY - pred + pg (fields 17..782: no borrow or carry across fields,
  // and only each field's value mod 256 is used below)
  const uint32_t pg = (pred >> 10) & 0xFFu;
  const uint32_t xk = X + LUMA_KY;
  const uint32_t t2 = (xk - pred) + (pg | (pg << 20));
  const bool l2 = has_up && (t2 & LUMA_MASK) == 0;
  // luma against 11 references, first hit wins (code.rs:293-339)
  uint32_t lk = 11u, lt = 0u;
  // (A/B: the search made unconditional on the fast path -- more VALU per
  // pixel -- was 6 % slower at 512 frames: whole waves often skip it)
  const bool need_luma = __builtin_amdgcn_ballot_w64(!br && !sd && !l2) != 0ull;
  if (need_luma) {
    // the wave issues first until its block's next tile barrier (as in the
    // slide kernel's classify_win: the block waits on its slowest wave)
    if constexpr (!HEAD) __builtin_amdgcn_s_setprio(1);
    const uint32_t refs[11] = {L, U, UR1, UR3, L3, VR1, V, VL1, UL3, VL3, VR3};
    if constexpr (HEAD) {
#pragma unroll
      for (int k = 10; k >= 0; --k) {
        const uint32_t t = xk - refs[k];
        const bool ok = (t & LUMA_MASK) == 0 && i > 0 && i >= (uint32_t)lr_rows(k) * W + (uint32_t)lr_px(k);
        lk = ok ? (uint32_t)k : lk;
        lt = ok ? t : lt;
      }
    } else {
      // first hit = min over k of ((t_k & LUMA_MASK) | k): the mask's lowest
      // bit is 32 > 10, so a miss keys >= 32 and a hit keys k (one v_and_or
      // per reference, v_min3 trees, no compare/select chains); the hit's
      // difference is taken again from the ring through the tile's address
      // table (ltab[k] = ring index of reference k for thread 0)
      uint32_t key[11];
#pragma unroll
      for (int k = 0; k < 11; ++k) key[k] = ((xk - refs[k]) & LUMA_MASK) | (uint32_t)k;
      const uint32_t m = min(min(min(min(key[0], key[1]), key[2]), min(min(key[3], key[4]), key[5])),
                             min(min(min(key[6], key[7]), key[8]), min(key[9], key[10])));
      lk = min(m, 11u);
      lt = xk - rbase[ltab[m & 15u] + tid];
    }
  }
  const uint32_t r = has_left ? d - K3(3u) : xr + K3(256u);   // = xr + 256 - pred per field
  // the record (nice_rec.hpp): BACK_REF and SMALL_DIFF onto the lane's
  // constant (mode range + absent slots); RGB's r, g, b fields (spread, 10-bit
  // spacing) to c0, s1, s2 by doubling g (one bit further up); LUMA2 / LUMA: g
  // (luma-space field 1) to c0 with the mode range (LUMA: + 64 k), r and b to
  // s1 and s2
  const uint32_t rec_br = (bk << 3) + cbr;
  const uint32_t rec_sd = (sdi << 3) + csd;
  const uint32_t rs = r & K3(0xFFu);
  const uint32_t rec_rgb = (rs + (rs & (0xFFu << 10))) << 3;
  const uint32_t lf = l2 ? t2 : lt;
  const uint32_t lbase = l2 ? ((C0_L2 << 3) | (SX_L2 << 14) | (SX_L2 << 23))
                            : ((C0_LUMA << 3) | (SX_LUMA << 14) | (SX_LUMA << 23)) + (lk << 9);
  const uint32_t rec_lu = lbase + (__builtin_amdgcn_ubfe(lf, 10, 6) << 3) + ((lf & 0x1Fu) << 14) +
                          ((lf & (0x1Fu << 20)) << 3);
  return br ? rec_br : sd ? rec_sd : (l2 || lk < 11u) ? rec_lu : rec_rgb;
}

// slot histogram (nice_rec.hpp) add of one record: three unconditional LDS
// adds (run members and absent slots land on the lane's own zero slots)
__device__ __forceinline__ void slot_hist_add(uint32_t* hs, uint32_t rec) {
  char* hb = reinterpret_cast<char*>(hs);
  atomicAdd(reinterpret_cast<uint32_t*>(hb + ((rec >> 1) & 0x1FFCu)), 1u);
  atomicAdd(reinterpret_cast<uint32_t*>(hb + C0_N * 4 + ((rec >> 12) & 0x7FCu)), 1u);
  atomicAdd(reinterpret_cast<uint32_t*>(hb + (C0_N + SX_N) * 4 + ((rec >> 21) & 0x7FCu)), 1u);
}

// RGB frames (C = 3, 4-byte aligned frames): a tile's 3072 bytes arrive as 768
// dwords (one or two per thread), are staged in LDS and each pixel's 3 bytes
// are taken with one funnel shift of two dwords.
constexpr int RGB_TILE_DW = ENC_TILE * 3 / 4;   // 768
__device__ __forceinline__ uint32_t rgb_dword(const uint8_t* fr, uint64_t nbytes, uint64_t j) {
  if (4 * j + 4 <= nbytes) return reinterpret_cast<const uint32_t*>(fr)[j];
  uint32_t v = 0;
  for (int k = 0; k < 4; ++k)
    if (4 * j + k < nbytes) v |= (uint32_t)fr[4 * j + k] << (8 * k);
  return v;
}
// pixel j of a frame as R | G << 8 | B << 16 (what y_from_rgba reads)
template <int C>
__device__ __forceinline__ uint32_t px_word(const uint8_t* fr, int64_t j) {
  if (C == 4) return reinterpret_cast<const uint32_t*>(fr)[j];
  const uint8_t* p = fr + 3 * j;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// ---------------------------------------------------------------------------
// The stages the ring, pair, slide, strip and twin bodies share.  Each LDS
// array stays declared in its body (the slide kernel places its own); these
// take pointers.  A stage with a barrier says so.
// ---------------------------------------------------------------------------
// The block's work items [w_begin, w_end): frame f, tile tt in [tile_lo,
// tile_hi) (frames: all tiles; bands: the band's).  False: none.
__device__ __forceinline__ bool cls_work_range(const EncArgs& a, uint64_t& w_begin, uint64_t& w_end) {
  const uint64_t total_work = (uint64_t)a.n_frames * (a.tile_hi - a.tile_lo);
  w_begin = (uint64_t)blockIdx.x * a.tiles_per_block;
  w_end = min(w_begin + a.tiles_per_block, total_work);
  return w_begin < w_end;
}
// The lane's record constants: BACK_REF / SMALL_DIFF ranges with absent slots,
// and the run-member record.
__device__ __forceinline__ void cls_lane_consts(uint32_t lane, uint32_t& cbr, uint32_t& csd, uint32_t& cunc) {
  cbr = (C0_BR << 3) | rec2_abs(lane);
  csd = (C0_SD << 3) | rec2_abs(lane);
  cunc = rec2_unc(lane);
}
// The slot histogram hs[C0_N + 2 SX_N] (nice_rec.hpp) and the run digits
// run_hist[8] (prefixes 5..12; RUNS = false: the kernel counts none).
template <bool RUNS = true>
__device__ __forceinline__ void cls_hist_zero(uint32_t* hs, uint32_t* run_hist) {
  for (uint32_t b = threadIdx.x; b < C0_N + 2 * SX_N; b += CLS_THREADS) hs[b] = 0;
  if constexpr (RUNS)
    if (threadIdx.x < 8) run_hist[threadIdx.x] = 0;
}
// The frame's symbol counts into the 858 bins (hfe.rs:29-45), once per block
// and frame.  A barrier before the counts are read; REZERO: a second one, then
// the counts start again from zero.
template <bool RUNS = true, bool REZERO = true>
__device__ __forceinline__ void cls_hist_flush(const EncArgs& a, uint32_t frame, uint32_t* hs, uint32_t* run_hist) {
  __syncthreads();
  for (int b = threadIdx.x; b < N_BINS; b += CLS_THREADS) {
    uint32_t v = slot_hist_bin(hs, b);
    if constexpr (RUNS)
      if (b >= BIN_PREFIX + P_RUN1 && b < BIN_PREFIX + P_RUN1 + 8) v += run_hist[b - BIN_PREFIX - P_RUN1];
    if (v) atomicAdd(&a.hist[(uint64_t)frame * N_BINS + b], v);
  }
  if constexpr (REZERO) {
    __syncthreads();
    cls_hist_zero<RUNS>(hs, run_hist);
  }
}
// Pixel i (Y space) into the ring, and into the guard past its end when it is
// one of the first CLS_GUARD words; uint4: pixels i .. i + 3, i % 4 == 0 (the
// slide kernel's; one template over the value type formed the scalar form's
// guard address with one more VALU instruction).
template <int RING>
__device__ __forceinline__ void cls_ring_put(uint32_t* ring, uint32_t i, uint32_t y) {
  const uint32_t k = i & (RING - 1);
  ring[k] = y;
  if (k < CLS_GUARD) ring[RING + k] = y;
}
template <int RING>
__device__ __forceinline__ void cls_ring_put(uint32_t* ring, uint32_t i, uint4 y) {
  const uint32_t k = i & (RING - 1);
  *reinterpret_cast<uint4*>(ring + k) = y;
  if (k < CLS_GUARD) *reinterpret_cast<uint4*>(ring + RING + k) = y;
}
// Pixels [lo, start) of frame fr into the ring: the 3 rows + 3 pixels before
// the block's first tile.  (The callers form lo: written here, 3 W lost its
// common subexpression with their `fast` test and the slide kernel changed.)
template <int C, int RING>
__device__ __forceinline__ void cls_ring_prefill(uint32_t* ring, int64_t lo, int64_t start, const uint8_t* fr) {
  for (int64_t j = lo + threadIdx.x; j < start; j += CLS_THREADS)
    cls_ring_put<RING>(ring, (uint32_t)j, y_from_rgba(px_word<C>(fr, j)));
}
// Tiles in the iteration starting at work item w (iterator ti): two when the
// next one is in the same frame and in the block's range.
__device__ __forceinline__ int cls_tiles_at(const TileIter& ti, uint64_t w, uint64_t w_end) {
  return (w + 1 < w_end && ti.k + 1 < ti.nt) ? 2 : 1;
}
// A wave's ballot of the coded flags of slot q (tile pixels q * CLS_THREADS +
// tid) into the tile's mask words; MASK_OUT: also into tile t's words of a.cmask
// (the address formed here, inside the branch: handed in as a pointer it
// stayed live across the tile and the _m ring kernels spilled two SGPRs).
template <bool MASK_OUT>
__device__ __forceinline__ void cls_flags_out(unsigned long long bal, uint32_t* mask, const EncArgs& a, uint64_t t,
                                              int q, int tid, int lane) {
  if (lane == 0) {
    const int wb = (q * CLS_THREADS + (tid & ~63)) >> 5;
    mask[wb] = (uint32_t)bal;
    mask[wb + 1] = (uint32_t)(bal >> 32);
    if constexpr (MASK_OUT) {
      uint32_t* cm = a.cmask + t * (ENC_TILE / 32);
      cm[wb] = (uint32_t)bal;
      cm[wb + 1] = (uint32_t)(bal >> 32);
    }
  }
}
// One whole wave, no loop: first / last coded pixel of tile t (pixels from
// `start`) out of its mask words.
__device__ __forceinline__ void cls_tile_edges(const uint32_t* mask, int64_t start, uint64_t t, const EncArgs& a,
                                               int lane) {
  const uint32_t mw = lane < ENC_TILE / 32 ? mask[lane] : 0u;
  const unsigned long long nz = __ballot(mw != 0);
  if (lane == 0) {
    uint32_t first = NONE, last = NONE;
    if (nz) {
      const int fw = __builtin_ctzll(nz), lw = 63 - __builtin_clzll(nz);
      first = (uint32_t)(start + fw * 32 + __builtin_ctz(mask[fw]));
      last = (uint32_t)(start + lw * 32 + 31 - __builtin_clz(mask[lw]));
    }
    a.tile_first[t] = first;
    a.tile_last[t] = last;
  }
}
// Run digits of the run after pixel p of a tile (count pixels, mask words;
// bal: the ballot of the lane's wave).  A run follows only if the next pixel
// is uncoded: most coded lanes stop at this one bit test (lane 63's next pixel
// is in the next wave: the mask).  Runs crossing the tile's end are
// enc_tailruns'.
__device__ __forceinline__ void cls_run_digits(uint32_t* run_hist, unsigned long long bal, int lane, int p, int count,
                                               const uint32_t* mask, bool coded) {
  const bool next_coded = lane < 63 && ((bal >> (lane + 1)) & 1ull);
  if (coded && !next_coded) {
    // next coded pixel: in this wave's 64 pixels from the ballot, else the tile mask
    const unsigned long long above = lane < 63 ? (bal >> (lane + 1)) : 0ull;
    const int nx = above ? p + 1 + (int)__builtin_ctzll(above) : next_coded_local(mask, p | 63);
    if (nx < count && nx > p + 1) {
      uint32_t mm = (uint32_t)(nx - p - 2);
      while (true) {
        atomicAdd(&run_hist[mm & 7u], 1u);
        if (mm < 8) break;
        mm >>= 3;
      }
    }
  }
}
// n linear pixels from g0 into registers, one per thread and k (0 outside
// [lo, hi): the frame / the caller's pixel memory): a row window of the strip
// and twin bodies.  (The callers form lo and hi: formed here, the strip
// kernel's code changed and its classify took 1.508 instead of 1.485 ms at
// 4 x 8192 x 8192, profiles/classify_refactor_ab.log.)
template <int C, int LD>
__device__ __forceinline__ void cls_window_load(uint32_t (&pw)[LD], const uint8_t* fr, int64_t g0, int n, int64_t lo,
                                                int64_t hi) {
#pragma unroll
  for (int k = 0; k < LD; ++k) {
    const int c = (int)threadIdx.x + k * CLS_THREADS;
    const int64_t g = g0 + c;
    pw[k] = (c < n && g >= lo && g < hi) ? px_word<C>(fr, g) : 0u;
  }
}

// MASK_OUT: as enc_classify_pair_body's (frames: coded flags out, run digits by
// enc_rundigits).
template <int C, int RING, bool MASK_OUT = false>
__device__ __forceinline__ void enc_classify_ring_body(const EncArgs& a) {
  __shared__ uint32_t ring[RING + CLS_GUARD];
  __shared__ uint32_t stage[C == 3 ? RGB_TILE_DW + 4 : 1];
  __shared__ uint32_t hs[C0_N + 2 * SX_N];     // slot histogram (nice_rec.hpp)
  __shared__ uint32_t run_hist[8];             // run digits (prefixes 5..12)
  __shared__ uint32_t mask[ENC_TILE / 32];
  __shared__ uint32_t ltab[2][CLS_PPT][16];   // [tile parity][q][luma reference]: ring index for thread 0
  uint64_t w_begin, w_end;
  if (!cls_work_range(a, w_begin, w_end)) return;
  const int tid = threadIdx.x, lane = tid & 63;
  uint32_t cbr, csd, cunc;
  cls_lane_consts((uint32_t)lane, cbr, csd, cunc);
  // back distance of luma reference k (code.rs:293-339), for the tile tables
  const uint32_t lback = tid < 16 * CLS_PPT && (tid & 15) < 11
                             ? (uint32_t)lr_rows(tid & 15) * a.W + (uint32_t)lr_px(tid & 15) : 0u;
  const uint32_t W = a.W;
  const int64_t N = (int64_t)W * a.H;
  cls_hist_zero(hs, run_hist);
  TileIter it(a, w_begin), nx(a, w_begin);
  uint32_t cur_frame = it.f;
  {
    const int64_t start = (int64_t)it.tt() * ENC_TILE;
    cls_ring_prefill<C, RING>(ring, max((int64_t)0, start - 3 * (int64_t)W - 3), start,
                              a.px + (uint64_t)cur_frame * a.frame_stride);
  }
  // the first tile's pixels
  uint32_t pf[CLS_PPT];
  auto fetch = [&](const TileIter& ti, uint32_t (&v)[CLS_PPT]) {
    const uint32_t f = ti.f;
    const int64_t start = (int64_t)ti.tt() * ENC_TILE;
    if (C == 4) {
      const uint32_t* fr = reinterpret_cast<const uint32_t*>(a.px + (uint64_t)f * a.frame_stride);
#pragma unroll
      for (int q = 0; q < CLS_PPT; ++q) {
        const int64_t j = start + q * CLS_THREADS + tid;
        v[q] = j < N ? fr[j] : 0u;
      }
    } else {   // the tile's dwords tid and 512 + tid
      const uint8_t* fr = a.px + (uint64_t)f * a.frame_stride;
      const uint64_t j0 = (uint64_t)ti.tt() * RGB_TILE_DW, nbytes = (uint64_t)N * 3;
      v[0] = 4 * (j0 + tid) < nbytes ? rgb_dword(fr, nbytes, j0 + tid) : 0u;
      v[1] = tid < RGB_TILE_DW - CLS_THREADS && 4 * (j0 + CLS_THREADS + tid) < nbytes
                 ? rgb_dword(fr, nbytes, j0 + CLS_THREADS + tid) : 0u;
    }
  };
  // two tiles in flight: tile w is staged from one register set while tiles
  // w + 1 (the other set) and w + 2 (refilling this one) load -- one tile of
  // classify work did not cover the HBM latency under load.  The loop body is
  // written once and instantiated for each set, so no register copy waits on
  // a load still in flight.
  uint32_t pb[CLS_PPT];
  fetch(nx, pf);
  nx.step(1);
  if (w_begin + 1 < w_end) fetch(nx, pb);
  nx.step(1);
  auto tile = [&](const uint64_t w, uint32_t (&pf)[CLS_PPT]) {
    const uint32_t f = it.f;
    const uint32_t tt = it.tt();
    if (f != cur_frame) {
      cls_hist_flush(a, cur_frame, hs, run_hist);
      cur_frame = f;
    }
    const int64_t start = (int64_t)tt * ENC_TILE;
    const int count = (int)min((int64_t)ENC_TILE, N - start);
    // stage this tile (Y space), start loading the next
    uint32_t pxw[CLS_PPT];
    if (C == 4) {
#pragma unroll
      for (int q = 0; q < CLS_PPT; ++q) pxw[q] = pf[q];
    } else {   // bytes via LDS: the previous tile's readers are past its staging barrier
      stage[tid] = pf[0];
      if (tid < RGB_TILE_DW - CLS_THREADS) stage[CLS_THREADS + tid] = pf[1];
      __syncthreads();
#pragma unroll
      for (int q = 0; q < CLS_PPT; ++q) {
        const uint32_t b = 3u * (uint32_t)(q * CLS_THREADS + tid);
        pxw[q] = __builtin_amdgcn_alignbit(stage[(b >> 2) + 1], stage[b >> 2], (b & 3u) * 8u);
      }
    }
    uint32_t yv[CLS_PPT];   // the thread's pixels in Y space (classify's X)
#pragma unroll
    for (int q = 0; q < CLS_PPT; ++q) {
      yv[q] = y_from_rgba(pxw[q]);
      cls_ring_put<RING>(ring, (uint32_t)(start + q * CLS_THREADS + tid), yv[q]);
    }
    // this tile's luma reference table (double-buffered: the previous tile's
    // readers are past the staging barrier below before it is rewritten)
    if (tid < 16 * CLS_PPT)
      ltab[w & 1][tid >> 4][tid & 15] =
          ((uint32_t)(start + (tid >> 4) * CLS_THREADS) - lback) & (RING - 1);
    if (w + 2 < w_end) fetch(nx, pf);
    nx.step(1);
    __syncthreads();
    __builtin_amdgcn_s_setprio(0);   // (raised by classify_y's luma search)
    // coded flags -> tile bitmask (a pixel is coded iff i == 0 or Y(i) != Y(i-1))
    uint32_t coded_bits = 0;
    unsigned long long wbal[CLS_PPT];   // coded flags of the wave's 64 pixels per q
#pragma unroll
    for (int q = 0; q < CLS_PPT; ++q) {
      const int p = q * CLS_THREADS + tid;
      const int64_t i = start + p;
      const uint32_t* bl = ring + ((uint32_t)(start + q * CLS_THREADS - 1) & (RING - 1)) + tid;
      const bool coded = p < count && (i == 0 || bl[1] != bl[0]);
      wbal[q] = __ballot(coded);
      cls_flags_out<MASK_OUT>(wbal[q], mask, a, it.tile(), q, tid, lane);
      coded_bits |= (coded ? 1u : 0u) << q;
    }
    __syncthreads();
    if (tid < 64) cls_tile_edges(mask, start, it.tile(), a, tid);
    const bool fast = start >= 3 * (int64_t)W + 3;
    uint32_t* recs = a.recs + (uint64_t)f * a.rec_stride + start;
    uint32_t rec[CLS_PPT];
#pragma unroll
    for (int q = 0; q < CLS_PPT; ++q) {   // both pixels' modes first (independent LDS reads)
      const int p = q * CLS_THREADS + tid;
      const bool coded = (coded_bits >> q) & 1u;
      uint32_t rf;
      if (fast)   // block-uniform: both variants are straight-line code
        rf = classify_ring<false, RING>(ring, (uint32_t)(start + q * CLS_THREADS), (uint32_t)tid, W, 0u, ltab[w & 1][q],
                                        cbr, csd, yv[q]);
      else
        rf = classify_ring<true, RING>(ring, (uint32_t)(start + q * CLS_THREADS), (uint32_t)tid, W, (uint32_t)(start + p),
                                       nullptr, cbr, csd, yv[q]);
      rec[q] = coded ? rf : cunc;
    }
#pragma unroll
    for (int q = 0; q < CLS_PPT; ++q) {
      const int p = q * CLS_THREADS + tid;
      const bool coded = (coded_bits >> q) & 1u;
      if (p < count) recs[p] = rec[q];
      // payload symbols (the mode prefixes are derived from them by enc_tables)
      slot_hist_add(hs, rec[q]);
      if constexpr (!MASK_OUT)   // (else enc_rundigits counts them)
        cls_run_digits(run_hist, wbal[q], lane, p, count, mask, coded);
    }
  };
  for (uint64_t w = w_begin; w < w_end; w += 2) {
    tile(w, pf);
    it.step(1);
    if (w + 1 < w_end) {
      tile(w + 1, pb);
      it.step(1);
    }
  }
  cls_hist_flush(a, cur_frame, hs, run_hist);
}
// ---------------------------------------------------------------------------
// K1p: the ring classify with up to two tiles per iteration ("pairs": 4
// pixels per thread, one staging barrier and one mask barrier per 2048
// pixels).  The pair is two consecutive tiles of one frame -- one contiguous
// 2048-pixel range of the raster -- so staging, coded flags and the mode
// decision run over it as one, with the per-tile outputs (first / last coded
// pixel, in-tile run digits) per tile; a tile left alone at a frame end or at
// the end of the block's range takes a one-tile iteration.  The next
// iteration's pixels load during this one (two tiles of work ahead).  The
// ring holds 3W + 3 pixels behind the pair plus the pair and the next one:
// 3W + 3 + 4096 <= RING.
// ---------------------------------------------------------------------------
// MASK_OUT (frames): the coded flags go out to a.cmask and enc_rundigits counts
// the run digits from them; false (bands): the digits are counted here.
template <int RING, bool MASK_OUT = false>
__device__ __forceinline__ void enc_classify_pair_body(const EncArgs& a) {
  constexpr int PQ = 2 * CLS_PPT;   // pixel slots per thread (4)
  __shared__ uint32_t ring[RING + CLS_GUARD];
  __shared__ uint32_t hs[C0_N + 2 * SX_N];     // slot histogram (nice_rec.hpp)
  __shared__ uint32_t run_hist[8];             // run digits (prefixes 5..12)
  __shared__ uint32_t mask[2 * ENC_TILE / 32];
  __shared__ uint32_t ltab[2][PQ][16];         // [iteration parity][q][luma reference]: ring index for thread 0
  uint64_t w_begin, w_end;
  if (!cls_work_range(a, w_begin, w_end)) return;
  const int tid = threadIdx.x, lane = tid & 63;
  uint32_t cbr, csd, cunc;
  cls_lane_consts((uint32_t)lane, cbr, csd, cunc);
  const uint32_t lback = tid < 16 * PQ && (tid & 15) < 11
                             ? (uint32_t)lr_rows(tid & 15) * a.W + (uint32_t)lr_px(tid & 15) : 0u;
  const uint32_t W = a.W;
  const int64_t N = (int64_t)W * a.H;
  cls_hist_zero(hs, run_hist);
  TileIter it(a, w_begin);
  uint32_t cur_frame = it.f;
  {
    const int64_t start = (int64_t)it.tt() * ENC_TILE;
    cls_ring_prefill<4, RING>(ring, max((int64_t)0, start - 3 * (int64_t)W - 3), start,
                              a.px + (uint64_t)cur_frame * a.frame_stride);
  }
  uint32_t pf[PQ];
  auto fetch = [&](const TileIter& ti, int nti) {
    const uint32_t* fr = reinterpret_cast<const uint32_t*>(a.px + (uint64_t)ti.f * a.frame_stride);
    const int64_t start = (int64_t)ti.tt() * ENC_TILE;
#pragma unroll
    for (int q = 0; q < PQ; ++q) {
      const int64_t j = start + q * CLS_THREADS + tid;
      pf[q] = (q < 2 * nti && j < N) ? fr[j] : 0u;
    }
  };
  uint64_t w = w_begin;
  int nti = cls_tiles_at(it, w, w_end);
  fetch(it, nti);
  uint32_t par = 0;
  while (w < w_end) {
    const int cur = nti;
    const uint32_t f = it.f;
    const uint32_t tt = it.tt();
    if (f != cur_frame) {
      cls_hist_flush(a, cur_frame, hs, run_hist);
      cur_frame = f;
    }
    const int64_t start = (int64_t)tt * ENC_TILE;
    const int count = (int)min((int64_t)(cur * ENC_TILE), N - start);   // pixels of the iteration
    // stage the iteration's pixels (Y space)
    uint32_t yv[PQ];   // the thread's pixels in Y space (classify's X)
#pragma unroll
    for (int q = 0; q < PQ; ++q) {
      yv[q] = y_from_rgba(pf[q]);
      if (q < 2 * cur) cls_ring_put<RING>(ring, (uint32_t)(start + q * CLS_THREADS + tid), yv[q]);
    }
    if (tid < 16 * PQ)
      ltab[par][tid >> 4][tid & 15] = ((uint32_t)(start + (tid >> 4) * CLS_THREADS) - lback) & (RING - 1);
    // the next iteration's pixels, in flight during this one
    TileIter nx = it;
    nx.step((uint32_t)cur);
    if (w + cur < w_end) {
      nti = cls_tiles_at(nx, w + cur, w_end);
      fetch(nx, nti);
    }
    __syncthreads();
    __builtin_amdgcn_s_setprio(0);   // (raised by classify_y's luma search)
    // coded flags -> bitmask (a pixel is coded iff i == 0 or Y(i) != Y(i-1))
    uint32_t coded_bits = 0;
    unsigned long long wbal[PQ];
#pragma unroll
    for (int q = 0; q < PQ; ++q) {
      const int p = q * CLS_THREADS + tid;
      const uint32_t* bl = ring + ((uint32_t)(start + q * CLS_THREADS - 1) & (RING - 1)) + tid;
      const bool coded = q < 2 * cur && p < count && ((start == 0 && p == 0) || bl[0] != yv[q]);
      wbal[q] = __ballot(coded);
      // (tiles tt, tt + 1 are consecutive: one 64-word range of masks)
      if (q < 2 * cur) cls_flags_out<MASK_OUT>(wbal[q], mask, a, it.tile(), q, tid, lane);
      coded_bits |= (coded ? 1u : 0u) << q;
    }
    __syncthreads();
    if (tid < 64 * cur) {   // wave j: first / last coded pixel of tile j
      const int j = tid >> 6;
      cls_tile_edges(mask + 32 * j, start + (int64_t)j * ENC_TILE, it.tile() + (uint64_t)j, a, lane);
    }
    const bool fast = start >= 3 * (int64_t)W + 3;
    uint32_t* recs = a.recs + (uint64_t)f * a.rec_stride + start;
    uint32_t rec[PQ];
    if (fast && cur == 2) {
      // the steady state (block-uniform): the four slots as one straight-line
      // block, so the scheduler interleaves their LDS reads and arithmetic
#pragma unroll
      for (int q = 0; q < PQ; ++q) {
        const uint32_t rf = classify_ring<false, RING>(ring, (uint32_t)(start + q * CLS_THREADS), (uint32_t)tid, W,
                                                       0u, ltab[par][q], cbr, csd, yv[q]);
        rec[q] = ((coded_bits >> q) & 1u) ? rf : cunc;
      }
    } else
#pragma unroll
    for (int q = 0; q < PQ; ++q) {   // every pixel's mode first (independent LDS reads)
      const int p = q * CLS_THREADS + tid;
      const bool coded = (coded_bits >> q) & 1u;
      uint32_t rf = cunc;
      if (q < 2 * cur) {   // block-uniform
        if (fast)
          rf = classify_ring<false, RING>(ring, (uint32_t)(start + q * CLS_THREADS), (uint32_t)tid, W, 0u,
                                          ltab[par][q], cbr, csd, yv[q]);
        else
          rf = classify_ring<true, RING>(ring, (uint32_t)(start + q * CLS_THREADS), (uint32_t)tid, W,
                                         (uint32_t)(start + p), nullptr, cbr, csd, yv[q]);
      }
      rec[q] = coded ? rf : cunc;
    }
#pragma unroll
    for (int q = 0; q < PQ; ++q) {
      if (q >= 2 * cur) continue;   // block-uniform
      const int p = q * CLS_THREADS + tid;
      const bool coded = (coded_bits >> q) & 1u;
      if (p < count) recs[p] = rec[q];
      slot_hist_add(hs, rec[q]);
      if constexpr (!MASK_OUT) {   // (else enc_rundigits counts them)
        const int j = q >> 1;      // the slot's tile: index and pixels in it
        cls_run_digits(run_hist, wbal[q], lane, p - j * ENC_TILE, min(count - j * ENC_TILE, ENC_TILE), mask + 32 * j,
                       coded);
      }
    }
    par ^= 1u;
    it.step((uint32_t)cur);
    w += (uint64_t)cur;
  }
  cls_hist_flush(a, cur_frame, hs, run_hist);
}

__global__ __launch_bounds__(CLS_THREADS) void enc_classify_ring(EncArgs a) { enc_classify_ring_body<4, CLS_RING>(a); }
__global__ __launch_bounds__(CLS_THREADS) void enc_classify_ring3(EncArgs a) { enc_classify_ring_body<3, CLS_RING>(a); }
__global__ __launch_bounds__(CLS_THREADS) void enc_classify_ring_m(EncArgs a) {
  enc_classify_ring_body<4, CLS_RING, true>(a);
}
__global__ __launch_bounds__(CLS_THREADS) void enc_classify_ring3_m(EncArgs a) {
  enc_classify_ring_body<3, CLS_RING, true>(a);
}
// a 32K-pixel ring (128 KB, one block per CU) for rows of up to
// CLS_RING2_MAX_W pixels: RGBA widths the strip kernel does not take (W %
// 1024 != 0, e.g. 7680 for 8K UHD) and RGB frames
__global__ __launch_bounds__(CLS_THREADS) void enc_classify_ring2(EncArgs a) { enc_classify_ring_body<4, 2 * CLS_RING>(a); }
__global__ __launch_bounds__(CLS_THREADS) void enc_classify_ring2_3(EncArgs a) { enc_classify_ring_body<3, 2 * CLS_RING>(a); }
__global__ __launch_bounds__(CLS_THREADS) void enc_classify_ring2_m(EncArgs a) {
  enc_classify_ring_body<4, 2 * CLS_RING, true>(a);
}
__global__ __launch_bounds__(CLS_THREADS) void enc_classify_ring2_3_m(EncArgs a) {
  enc_classify_ring_body<3, 2 * CLS_RING, true>(a);
}
// pairs of tiles per iteration (16K ring: W <= CLS_PAIR_MAX_W)
// (RGBA; an RGB pair's 6 KB byte stage would push the block past 80 KB of LDS,
// one block per CU)
__global__ __launch_bounds__(CLS_THREADS, 2) void enc_classify_pair(EncArgs a) { enc_classify_pair_body<CLS_RING>(a); }
__global__ __launch_bounds__(CLS_THREADS, 2) void enc_classify_pair_m(EncArgs a) {
  enc_classify_pair_body<CLS_RING, true>(a);
}

// ---------------------------------------------------------------------------
// K1w: classify with per-lane sliding windows (round 6; RGBA frames, 3 <= W <=
// CLS_PAIR_MAX_W, pixel memory 16-byte aligned: the bench path).  The pair
// kernel gives each lane pixels 512 apart, so every pixel re-reads its 13
// neighbours from the ring one word at a time (about 15 LDS instructions and
// three Y -> RGB conversions per pixel).  Here a lane owns 4 CONSECUTIVE
// pixels of the iteration's 2048 (one 16-byte global load, one 16-byte ring
// store) and reads, per neighbour row, one aligned window covering its 4
// pixels' references (rows y-1 and y-3: pixels i-rW-3 .. i-rW+6; row y-2:
// i-2W .. i-2W+3; row y: the 3 pixels before) with ds_read_b128s -- 8 to 11
// per 4 pixels, conflict-free (consecutive lanes read consecutive 16 bytes).
// Every reference is then a register chosen at compile time: the window
// offsets depend only on W mod 4 (the template parameter), the left
// neighbours L, L2, L3 of pixels 1..3 are the lane's own pixels, and pixel
// q's RGB spread is pixel q+1's RGB(L) (one conversion saved per pixel).
// The coded flags come out of the compares as wave ballots; the per-tile
// first / last coded pixel are found from them with scalar bit scans, and the
// flags go to a.cmask in the ballot order (wave w's 8 words: ballot q's low
// and high halves), which enc_rundigits transposes.  Same records, histogram
// and tile edges as enc_classify_pair_m (code.rs:159-414).
// ---------------------------------------------------------------------------
// pixel word v (R | G << 8 | B << 16) -> its Y-space value and RGB spread (sharing G)
__device__ __forceinline__ void y_rgb_from_rgba(uint32_t v, uint32_t& y, uint32_t& xr) {
  const uint32_t g = __builtin_amdgcn_ubfe(v, 8, 8);
  const nice_u16x2 d = __builtin_bit_cast(nice_u16x2, v) - __builtin_bit_cast(nice_u16x2, g | (g << 16));
  const uint32_t t = __builtin_bit_cast(uint32_t, d);
  y = (__umul24(t & 0xFF0000u, 16u) + (t & 0xFFu)) | (g << 10);
  xr = (y + __umul24(g, 0x100001u)) & K3(0xFFu);
}

// classify_y<false> with every reference in registers: X (Y space) and its RGB
// spread xr, L and its spread lrgb; the luma hit's difference is read again from
// the ring at byte (i4 + loff4[k]) mod 4 RING (i4 = 4 i, loff4[k] = -4 offset of
// reference k).
__device__ __forceinline__ uint32_t classify_win(uint32_t X, uint32_t xr, uint32_t L, uint32_t lrgb, uint32_t L2,
                                                 uint32_t L3, uint32_t U, uint32_t UR1, uint32_t UR3, uint32_t UL3,
                                                 uint32_t U2, uint32_t V, uint32_t VR1, uint32_t VL1, uint32_t VL3,
                                                 uint32_t VR3, const uint32_t* ring, uint32_t i4, const uint32_t* loff4,
                                                 uint32_t cbr, uint32_t csd, uint32_t pq) {
  // back references k = 1..4 (code.rs:191-206)
  const bool e1 = U == X, e2 = UR1 == X, e3 = L2 == X, e4 = U2 == X;
  const bool br = e1 | e2 | e3 | e4;
  const uint32_t bk = e1 ? 1u : e2 ? 2u : e3 ? 3u : 4u;
  const uint32_t pred = avg3(rgb_from_y(U), lrgb);
  // small diff (code.rs:208-247), as in classify_y
  const uint32_t d = xr + K3(259u) - pred;
  const bool sd = ((d & K3(0x3F8u)) | ((d + K3(1u)) & K3(8u))) == K3(0x100u);
  const uint32_t sdi = (__umul24(d & K3(7u), 49u | (7u << 10) | (1u << 20)) >> 20) & 0x3FFu;
  // luma2 (code.rs:252-292)
  const uint32_t pg = (pred >> 10) & 0xFFu;
  const uint32_t xk = X + LUMA_KY;
  const uint32_t t2 = (xk - pred) + (pg | (pg << 20));
  const bool l2 = (t2 & LUMA_MASK) == 0;
  // luma, 11 references, first hit wins (code.rs:293-339): min-key search
  uint32_t lk = 11u, lt = 0u;
  if (__builtin_amdgcn_ballot_w64(!br && !sd && !l2) != 0ull) {
    // a wave that takes the luma search issues first until its block's next
    // barrier (the block waits on its slowest wave), the more so the later in
    // the lane's four pixels it needs it (pq: 1, 1, 2, 3): classify 15.22 ->
    // 14.12 ms per 512 frames (profiles/r06zp_ab_cls_prio.log,
    // r06zq_ab_cls_prio_modes.log; by the count of searches so far: 14.35)
    if (pq >= 3) __builtin_amdgcn_s_setprio(3);
    else if (pq == 2) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(1);
    const uint32_t refs[11] = {L, U, UR1, UR3, L3, VR1, V, VL1, UL3, VL3, VR3};
    uint32_t key[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) key[k] = ((xk - refs[k]) & LUMA_MASK) | (uint32_t)k;
    const uint32_t m = min(min(min(min(key[0], key[1]), key[2]), min(min(key[3], key[4]), key[5])),
                           min(min(min(key[6], key[7]), key[8]), min(key[9], key[10])));
    lk = min(m, 11u);
    // loff4[k]: -4 (offset of reference k) mod 4 RING bytes (0 at k = 11)
    lt = xk - *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(ring) +
                                                  ((i4 + loff4[lk]) & ((CLS_RING - 1) * 4)));
  }
  const uint32_t r = d - K3(3u);   // = xr + 256 - pred per field
  const uint32_t rec_br = (bk << 3) + cbr;
  const uint32_t rec_sd = (sdi << 3) + csd;
  const uint32_t rs = r & K3(0xFFu);
  const uint32_t rec_rgb = (rs + (rs & (0xFFu << 10))) << 3;
  const uint32_t lf = l2 ? t2 : lt;
  const uint32_t lbase = l2 ? ((C0_L2 << 3) | (SX_L2 << 14) | (SX_L2 << 23))
                            : ((C0_LUMA << 3) | (SX_LUMA << 14) | (SX_LUMA << 23)) + (lk << 9);
  const uint32_t rec_lu = lbase + (__builtin_amdgcn_ubfe(lf, 10, 6) << 3) + ((lf & 0x1Fu) << 14) +
                          ((lf & (0x1Fu << 20)) << 3);
  return br ? rec_br : sd ? rec_sd : (l2 || lk < 11u) ? rec_lu : rec_rgb;
}

// a lane's records past the frame's end are not stored (1..3 of its 4 remain)
__device__ __noinline__ void store_tail3(uint32_t* p, uint32_t r0, uint32_t r1, uint32_t r2, int n) {
  p[0] = r0;
  if (n > 1) p[1] = r1;
  if (n > 2) p[2] = r2;
}

template <int WM>   // W mod 4
__device__ __forceinline__ void enc_classify_slide_body(const EncArgs& a) {
  constexpr int RING = CLS_RING;
  constexpr uint32_t RM = RING - 1;
  // window geometry (words, all multiples of 4 away from the lane's first
  // pixel i0 = start + 4 tid): row r's window starts OFF_r before i0, rounded
  // up to a multiple of 4 by D_r, and spans NB_r 16-byte blocks
  constexpr uint32_t D1 = (4u - (uint32_t)(WM + 3) % 4u) % 4u;       // row y-1: i - W - 3 ..
  constexpr uint32_t D2 = (4u - (uint32_t)(2 * WM) % 4u) % 4u;       // row y-2: i - 2W ..
  constexpr uint32_t D3 = (4u - (uint32_t)(3 * WM + 3) % 4u) % 4u;   // row y-3: i - 3W - 3 ..
  constexpr int NB1 = (int)(D1 + 10u + 3u) / 4, NB2 = (int)(D2 + 4u + 3u) / 4, NB3 = (int)(D3 + 10u + 3u) / 4;
  // one block of LDS, laid out so that the histogram sits at address 0: its
  // atomics' base folds into the instruction's 16-bit offset (placed after
  // the 67 KB ring it cost one VALU add per atomic, three per pixel)
  struct SlideLds {
    uint32_t hs[C0_N + 2 * SX_N];               // slot histogram (nice_rec.hpp)
    uint32_t loff4[16];                         // luma reference k: -4 (its offset) mod 4 RING
    uint32_t wfl[2][CLS_THREADS / 64][2];       // [parity][wave]: first coded pixel, last + 1 (tile-relative)
    __attribute__((aligned(16))) uint32_t ring[RING + CLS_GUARD];
  };
  __shared__ SlideLds sl;
  uint32_t* const hs = sl.hs;
  uint32_t* const loff4 = sl.loff4;
  uint32_t* const ring = sl.ring;
  auto& wfl = sl.wfl;
  uint64_t w_begin, w_end;
  if (!cls_work_range(a, w_begin, w_end)) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t cbr, csd, cunc;
  cls_lane_consts(lane, cbr, csd, cunc);
  const uint32_t W = a.W;
  const int64_t N = (int64_t)W * a.H;
  const uint32_t OFF1 = W + 3u + D1, OFF2 = 2u * W + D2, OFF3 = 3u * W + 3u + D3;
  cls_hist_zero<false>(hs, nullptr);   // (run digits: enc_rundigits)
  if (tid < 16)
    loff4[tid] = tid < 11 ? ((0u - ((uint32_t)lr_rows((int)tid) * W + (uint32_t)lr_px((int)tid))) & RM) * 4u : 0u;
  TileIter it(a, w_begin);
  uint32_t cur_frame = it.f;
  {
    const int64_t start = (int64_t)it.tt() * ENC_TILE;
    cls_ring_prefill<4, RING>(ring, max((int64_t)0, start - 3 * (int64_t)W - 3), start,
                              a.px + (uint64_t)cur_frame * a.frame_stride);
  }
  uint4 pf;
  auto fetch = [&](const TileIter& ti, int nti) {
    const uint32_t* fr = reinterpret_cast<const uint32_t*>(a.px + (uint64_t)ti.f * a.frame_stride);
    const int64_t j = (int64_t)ti.tt() * ENC_TILE + 4 * (int64_t)tid;
    if (tid < 256u * (uint32_t)nti && j + 4 <= N) {
      pf = *reinterpret_cast<const uint4*>(fr + j);
    } else {
      const bool in = tid < 256u * (uint32_t)nti;
      pf.x = in && j < N ? fr[j] : 0u;
      pf.y = in && j + 1 < N ? fr[j + 1] : 0u;
      pf.z = in && j + 2 < N ? fr[j + 2] : 0u;
      pf.w = in && j + 3 < N ? fr[j + 3] : 0u;
    }
  };
  // the previous iteration's tiles: first / last coded pixel from its waves'
  // entries (after a barrier)
  uint64_t prev_tile = 0;
  int64_t prev_start = 0;
  uint32_t prev_cur = 0, prev_par = 0;
  auto combine = [&]() {
    if (tid < prev_cur) {
      uint32_t fi = NONE, la = 0;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        fi = min(fi, wfl[prev_par][4 * tid + v][0]);
        la = max(la, wfl[prev_par][4 * tid + v][1]);
      }
      const int64_t sj = prev_start + (int64_t)tid * ENC_TILE;
      a.tile_first[prev_tile + tid] = fi == NONE ? NONE : (uint32_t)(sj + fi);
      a.tile_last[prev_tile + tid] = la == 0 ? NONE : (uint32_t)(sj + la - 1);
    }
  };
  uint64_t w = w_begin;
  int nti = cls_tiles_at(it, w, w_end);
  fetch(it, nti);
  uint32_t par = 0;
  while (w < w_end) {
    const int cur = nti;
    const uint32_t f = it.f;
    if (f != cur_frame) {
      cls_hist_flush<false>(a, cur_frame, hs, nullptr);
      cur_frame = f;
    }
    const int64_t start = (int64_t)it.tt() * ENC_TILE;
    const int count = (int)min((int64_t)(cur * ENC_TILE), N - start);   // pixels of the iteration
    // the lane's 4 pixels in Y space and RGB spread; into the ring
    uint32_t X[4], XR[4];
    y_rgb_from_rgba(pf.x, X[0], XR[0]);
    y_rgb_from_rgba(pf.y, X[1], XR[1]);
    y_rgb_from_rgba(pf.z, X[2], XR[2]);
    y_rgb_from_rgba(pf.w, X[3], XR[3]);
    const uint32_t i0 = (uint32_t)start + 4u * tid;
    if (tid < 256u * (uint32_t)cur) cls_ring_put<RING>(ring, i0, make_uint4(X[0], X[1], X[2], X[3]));
    // the next iteration's pixels, in flight during this one
    TileIter nx = it;
    nx.step((uint32_t)cur);
    if (w + cur < w_end) {
      nti = cls_tiles_at(nx, w + cur, w_end);
      fetch(nx, nti);
    }
    __syncthreads();
    __builtin_amdgcn_s_setprio(0);   // (raised by classify_win's luma search)
    if (prev_cur) combine();
    const bool fast = start >= 3 * (int64_t)W + 3;   // block-uniform
    uint32_t rec[4];
    unsigned long long bal[4];
    if (fast) {
      // the windows: base = ring index of (wave's first pixel - OFF_r) plus 4 lane
      const uint32_t sw = (uint32_t)start + 256u * wave;
      const uint32_t i4 = 4u * i0;
      const uint32_t* b0 = ring + ((sw - 4u) & RM) + 4u * lane;
      const uint32_t* b1 = ring + ((sw - OFF1) & RM) + 4u * lane;
      const uint32_t* b2 = ring + ((sw - OFF2) & RM) + 4u * lane;
      const uint32_t* b3 = ring + ((sw - OFF3) & RM) + 4u * lane;
      uint32_t w0[4], w1[4 * NB1], w2[4 * NB2], w3[4 * NB3];
      // whole 16-byte blocks (ds_read_b128: conflict-free for consecutive
      // lanes); the empty asm keeps the compiler from narrowing a block whose
      // end words are unused into ds_read2_b64 / b32 pieces, which conflict
      // two-way at this 16-byte lane stride (classify 15.95 -> 15.39 ms per
      // 512 4K frames)
      auto blk = [](const uint32_t* p, uint32_t* d) {
        nice_u32x4 v = *reinterpret_cast<const nice_u32x4*>(p);
        asm volatile("" : "+v"(v));
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      };
      blk(b0, w0);
#pragma unroll
      for (int b = 0; b < NB1; ++b) blk(b1 + 4 * b, w1 + 4 * b);
#pragma unroll
      for (int b = 0; b < NB2; ++b) blk(b2 + 4 * b, w2 + 4 * b);
#pragma unroll
      for (int b = 0; b < NB3; ++b) blk(b3 + 4 * b, w3 + 4 * b);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t L = q >= 1 ? X[q - 1] : w0[3];
        const uint32_t L2 = q >= 2 ? X[q - 2] : w0[2 + q];
        const uint32_t L3 = q >= 3 ? X[q - 3] : w0[1 + q];
        const uint32_t lrgb = q >= 1 ? XR[q - 1] : rgb_from_y(w0[3]);
        const uint32_t pq = q == 3 ? 3u : q == 2 ? 2u : 1u;   // (compile-time after unrolling)
        const uint32_t rf = classify_win(X[q], XR[q], L, lrgb, L2, L3, w1[q + 3 + D1], w1[q + 4 + D1],
                                         w1[q + 6 + D1], w1[q + D1], w2[q + D2], w3[q + 3 + D3], w3[q + 4 + D3],
                                         w3[q + 2 + D3], w3[q + D3], w3[q + 6 + D3], ring, i4 + 4u * (uint32_t)q,
                                         loff4, cbr, csd, pq);
        // (the flag after the decision: kept across it, it went through a VGPR)
        const bool coded = 4 * (int)tid + q < count && X[q] != L;
        bal[q] = __builtin_amdgcn_ballot_w64(coded);
        rec[q] = coded ? rf : cunc;
      }
    } else {
      // the frame's first rows: the reference's validity rules (classify_y<true>)
      // per pixel, neighbours one word at a time (s + tid: the pixel's index)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t i = i0 + (uint32_t)q;
        const bool coded = 4 * (int)tid + q < count && (i == 0 || X[q] != ring[(i - 1u) & RM]);
        bal[q] = __builtin_amdgcn_ballot_w64(coded);
        const uint32_t rf = classify_ring<true>(ring, (uint32_t)start + (uint32_t)q + 3u * tid, tid, W, i, nullptr,
                                                cbr, csd, X[q]);
        rec[q] = coded ? rf : cunc;
      }
    }
    // the wave's first / last coded pixel (tile-relative) and its coded flags
    // in ballot order (enc_rundigits transposes them)
    if (tid < 256u * (uint32_t)cur) {
      uint32_t fi = NONE, la = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (bal[q]) {
          fi = min(fi, 4u * (uint32_t)__builtin_ctzll(bal[q]) + (uint32_t)q);
          la = max(la, 4u * (uint32_t)(63 - __builtin_clzll(bal[q])) + (uint32_t)q + 1u);
        }
      }
      const uint32_t wo = 256u * (wave & 3u);
      if (lane == 0) {
        wfl[par][wave][0] = fi == NONE ? NONE : wo + fi;
        wfl[par][wave][1] = la == 0 ? 0u : wo + la;
      }
      const uint32_t hw = lane & 1u, qq = (lane >> 1) & 3u;
      const unsigned long long bq = qq == 0 ? bal[0] : qq == 1 ? bal[1] : qq == 2 ? bal[2] : bal[3];
      if (lane < 8u) a.cmask[(it.tile() + (wave >> 2)) * (ENC_TILE / 32) + 8u * (wave & 3u) + lane] =
          (uint32_t)(bq >> (32u * hw));
    }
    // records out (one 16-byte store; a lane with pixels past the frame's end
    // stores them one by one), histogram
    uint32_t* recs = a.recs + (uint64_t)f * a.rec_stride + (uint64_t)i0;
    if (4 * (int)tid + 3 < count)
      *reinterpret_cast<uint4*>(__builtin_assume_aligned(recs, 16)) = make_uint4(rec[0], rec[1], rec[2], rec[3]);
    else if (4 * (int)tid < count)
      store_tail3(recs, rec[0], rec[1], rec[2], count - 4 * (int)tid);
    if (tid < 256u * (uint32_t)cur) {
#pragma unroll
      // (same-address adds cost nothing extra: every lane on its own zero
      // slots instead measured slower, 14.07 -> 14.74 ms, r06zt_hist_probe.log)
      for (int q = 0; q < 4; ++q) slot_hist_add(hs, rec[q]);
    }
    prev_tile = it.tile();
    prev_start = start;
    prev_cur = (uint32_t)cur;
    prev_par = par;
    par ^= 1u;
    it.step((uint32_t)cur);
    w += (uint64_t)cur;
  }
  __syncthreads();
  combine();
  cls_hist_flush<false>(a, cur_frame, hs, nullptr);
}
__global__ __launch_bounds__(CLS_THREADS, 2) void enc_classify_slide0(EncArgs a) { enc_classify_slide_body<0>(a); }
__global__ __launch_bounds__(CLS_THREADS, 2) void enc_classify_slide1(EncArgs a) { enc_classify_slide_body<1>(a); }
__global__ __launch_bounds__(CLS_THREADS, 2) void enc_classify_slide2(EncArgs a) { enc_classify_slide_body<2>(a); }
__global__ __launch_bounds__(CLS_THREADS, 2) void enc_classify_slide3(EncArgs a) { enc_classify_slide_body<3>(a); }

// ---------------------------------------------------------------------------
// K1r: run digits of the runs inside tiles (code.rs:371-407: a run between two
// coded pixels of one tile, length L >= 1, adds the base-8 digits of L - 1 to
// the run prefixes' bins; runs that cross a tile's end are enc_tailruns'),
// from the coded flags enc_classify_pair_m wrote, one 32-pixel word per lane.
// Counting them inside the classify loop cost that loop 17 % (21.2 vs 17.5 ms
// per 512 4K frames without the block), in its branches and live state.  A
// run ends at each coded pixel whose previous pixel is uncoded; its start is
// the previous coded pixel of the word, or the last coded pixel of the tile's
// earlier words (a max scan over the half-wave), or none in the tile (skipped).
// ---------------------------------------------------------------------------
// il != 0: the tiles' flags are in enc_classify_slide's ballot order (wave w
// of a tile: words 8w + 2q + h = half h of the ballot of its lanes' q-th
// pixels, pixel 256w + 4 lane + q), transposed here: standard word k holds
// byte k % 8 of each ballot q, bit m at 4m + q.
__global__ __launch_bounds__(RUNDIGITS_THREADS) void enc_rundigits(EncArgs a, int il) {
  __shared__ uint32_t bins[8];
  if (threadIdx.x < 8) bins[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t f = blockIdx.y, T = a.tiles_per_frame;
  const uint32_t lane = threadIdx.x & 63u, k = lane & 31u;
  const uint32_t wv = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwv = gridDim.x * (blockDim.x >> 6);
  uint32_t cnt[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  // RD_U tile pairs per iteration, every load issued before any is used (one
  // pair per iteration waited on each load: 0.65 ms per 512 4K frames)
  constexpr uint32_t RD_U = 4;
  for (uint32_t tb0 = 2u * wv; tb0 < T; tb0 += 2u * nwv * RD_U) {
    uint32_t raw[RD_U][4];
#pragma unroll
    for (uint32_t u = 0; u < RD_U; ++u) {
      const uint32_t t = tb0 + 2u * nwv * u + (lane >> 5);   // lanes 0-31: the pair's first tile, 32-63: its second
      const uint32_t* tw = a.cmask + ((uint64_t)f * T + (t < T ? t : 0u)) * (ENC_TILE / 32);
      if (il) {
        tw += 8u * (k >> 3) + ((k >> 2) & 1u);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) raw[u][q] = t < T ? tw[2 * q] : 0u;
      } else {
        raw[u][0] = t < T ? tw[k] : 0u;
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < RD_U; ++u) {
    const uint32_t t = tb0 + 2u * nwv * u + (lane >> 5);
    if (__all(t >= T)) break;   // (wave-uniform: the pairs past the frame's tiles)
    uint32_t m = 0;
    if (t < T) {
      if (il) {
        const uint32_t sh = 8u * (k & 3u);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
          uint32_t x = (raw[u][q] >> sh) & 0xFFu;   // bit m -> bit 4m
          x = (x | (x << 12)) & 0x000F000Fu;
          x = (x | (x << 6)) & 0x03030303u;
          x = (x | (x << 3)) & 0x11111111u;
          m |= x << q;
        }
        // the standard order back in place (enc_pack reads 16 flags per lane
        // from it); every source word of the tile was read by this wave's
        // loads above
        a.cmask[((uint64_t)f * T + t) * (ENC_TILE / 32) + k] = m;
      } else {
        m = raw[u][0];
      }
    }
    // last coded pixel of the tile before this word (-1: none)
    int inc = m ? (int)(32u * k + 31u - (uint32_t)__clz((int)m)) : -1;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
      const int v = __shfl_up(inc, o);
      if ((int)k >= o) inc = max(inc, v);
    }
    int before = __shfl_up(inc, 1);
    uint32_t pm = __shfl_up(m, 1);
    if (k == 0u) { before = -1; pm = 0x80000000u; }   // (a run into the tile: not counted here)
    uint32_t tb = m & ~((m << 1) | (pm >> 31));        // coded pixels after an uncoded one
    while (tb) {
      const uint32_t b = (uint32_t)__builtin_ctz(tb);
      tb &= tb - 1u;
      const uint32_t below = m & ((1u << b) - 1u);
      const int prev = below ? (int)(32u * k + 31u - (uint32_t)__clz((int)below)) : before;
      if (prev >= 0) {
        uint32_t mm = (uint32_t)((int)(32u * k + b) - prev - 2);
        while (true) {
          const uint32_t d = mm & 7u;
#pragma unroll
          for (int j = 0; j < 8; ++j) cnt[j] += d == (uint32_t)j ? 1u : 0u;
          if (mm < 8u) break;
          mm >>= 3;
        }
      }
    }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {   // wave sums, then one LDS add per wave and bin
    uint32_t v = cnt[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0 && v) atomicAdd(&bins[j], v);
  }
  __syncthreads();
  if (threadIdx.x < 8 && bins[threadIdx.x])
    atomicAdd(&a.hist[(uint64_t)f * N_BINS + BIN_PREFIX + P_RUN1 + threadIdx.x], bins[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// K1s: classify, strip-staged (RGBA frames with W % 1024 == 0 too wide for the
// ring: W > CLS_RING_MAX_W).  The frame is cut into vertical strips of up to
// STRIP_W columns (a multiple of 1024, so each strip row is whole raster tiles
// and the tile bookkeeping is the ring kernel's); a block walks rows
// [y0, y1) of one strip keeping four row windows in LDS, each the LINEAR
// pixels [yW + x0 - 3, yW + x1 + 3) of its row: every reference of a pixel
// of the strip -- 0..3 rows up, 3 pixels either side, wrapping across row ends
// like the reference's linear offsets (code.rs:141-145) -- is inside the
// window of its row.  Same outputs as enc_classify_ring.
// ---------------------------------------------------------------------------
// (STRIP_W: nice_geom.h)
constexpr int STRIP_RS = STRIP_W + 8;              // window words (+3 each side, padded)
constexpr int STRIP_LD = (STRIP_W + 6 + CLS_THREADS - 1) / CLS_THREADS;   // window loads per thread (5)

template <bool MASK_OUT>
__device__ __forceinline__ void enc_classify_strip_body(const EncArgs& a) {
  __shared__ uint32_t win[4][STRIP_RS];
  __shared__ uint32_t hs[C0_N + 2 * SX_N];
  __shared__ uint32_t run_hist[8];
  __shared__ uint32_t mask[STRIP_W / ENC_TILE][ENC_TILE / 32];
  __shared__ uint32_t ltab[STRIP_W / ENC_TILE][CLS_PPT][16];
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t W = a.W, H = a.H;
  const uint32_t T = a.tiles_per_frame, tpr = W / ENC_TILE;   // tiles per row
  const uint32_t nstrips = (W + STRIP_W - 1) / STRIP_W;
  const uint32_t rows = a.tiles_per_block;                    // rows per block
  // the band's rows (frames: all)
  const uint32_t ylo = a.tile_lo / tpr, yhi = (a.tile_hi + tpr - 1) / tpr;
  const uint32_t nchunks = (yhi - ylo + rows - 1) / rows;
  uint32_t b = blockIdx.x;
  const uint32_t chunk = b % nchunks;
  b /= nchunks;
  const uint32_t s = b % nstrips, f = b / nstrips;
  if (f >= a.n_frames) return;
  const uint32_t y0 = ylo + chunk * rows, y1 = min(y0 + rows, yhi);
  const uint32_t x0 = s * STRIP_W, x1 = min(x0 + STRIP_W, W);
  const uint32_t ntr = (x1 - x0) / ENC_TILE;                  // tiles per strip row (1 or 2)
  const uint8_t* fr = a.px + (uint64_t)f * a.frame_stride;
  const int64_t N = (int64_t)W * H;
  uint32_t cbr, csd, cunc;
  cls_lane_consts((uint32_t)lane, cbr, csd, cunc);
  cls_hist_zero(hs, run_hist);
  // row y's window: linear pixels [yW + x0 - 3, yW + x1 + 3), loaded into registers
  uint32_t pw[STRIP_LD];
  auto fetch_row = [&](int64_t y) {   // y = -1: the window of row -1 (its end is row 0's first pixels)
    const int64_t lo = max((int64_t)0, a.px_lo), hi = min(N, a.px_hi);
    cls_window_load<4>(pw, fr, y * (int64_t)W + x0 - 3, (int)(x1 - x0) + 6, lo, hi);
  };
  auto commit_row = [&](int64_t y) {
    uint32_t* wr = win[(uint32_t)y & 3u];
#pragma unroll
    for (int k = 0; k < STRIP_LD; ++k) {
      const int c = tid + k * CLS_THREADS;
      if (c < (int)(x1 - x0) + 6) wr[c] = y_from_rgba(pw[k]);
    }
  };
  // prefill rows y0-3 .. y0-1, from row -1 on: the window of the row above
  // row 0 ends with row 0's first pixels, which the last columns of row 0
  // reference through offsets W-1 and W-3 (code.rs:141-145; round 5 width
  // sweep: 10240 x 12 RGBA frames whose pixel W-3 only luma reference 3 predicts)
  for (int64_t y = y0 >= 3 ? (int64_t)y0 - 3 : -1; y < (int64_t)y0; ++y) {
    fetch_row(y);
    commit_row(y);
  }
  // back distance of luma reference k in (rows, pixels) for the tile tables
  const int lk_rows = tid < 16 && tid < 11 ? lr_rows(tid) : 0, lk_px = tid < 16 && tid < 11 ? lr_px(tid) : 0;
  fetch_row(y0);
  for (uint32_t y = y0; y < y1; ++y) {
    // row y's window replaces row y - 4's, which row y - 1 still references:
    // every thread is past row y - 1 first (also for ltab and mask)
    __syncthreads();
    commit_row(y);
    if (y + 1 < y1) fetch_row(y + 1);
    // luma reference tables: window index of reference k for thread 0 of
    // (tile j, q); the window of row y - r holds column x at x - x0 + 3
    if (tid < 16) {
      for (uint32_t j = 0; j < ntr; ++j)
#pragma unroll
        for (int q = 0; q < CLS_PPT; ++q)
          ltab[j][q][tid] = ((y - (uint32_t)lk_rows) & 3u) * STRIP_RS +
                            (uint32_t)((int)(j * ENC_TILE + q * CLS_THREADS) + 3 - lk_px);
    }
    __syncthreads();
    // (no s_setprio(0) here, unlike ring / pair / slide: a scheduling change, wants an A/B of its own)
    // coded flags of the row's tiles
    uint32_t coded_bits = 0;
    unsigned long long wbal[2][CLS_PPT];
    const uint32_t* wy = win[y & 3];
    for (uint32_t j = 0; j < ntr; ++j) {
#pragma unroll
      for (int q = 0; q < CLS_PPT; ++q) {
        const int c = (int)(j * ENC_TILE) + q * CLS_THREADS + tid;   // column in the strip
        const int64_t i = (int64_t)y * W + x0 + c;
        const bool coded = i == 0 || wy[c + 3] != wy[c + 2];
        wbal[j][q] = __ballot(coded);
        // (frames: every tile is the block's)
        cls_flags_out<MASK_OUT>(wbal[j][q], mask[j], a, (uint64_t)f * T + (y * W + x0) / ENC_TILE + j, q, tid, lane);
        coded_bits |= (coded ? 1u : 0u) << (2 * j + q);
      }
    }
    __syncthreads();
    for (uint32_t j = 0; j < ntr; ++j) {
      const uint32_t tt = (y * W + x0) / ENC_TILE + j;   // raster tile
      const bool in_band = tt >= a.tile_lo && tt < a.tile_hi;   // block-uniform
      const int64_t start = (int64_t)tt * ENC_TILE;
      // first / last coded pixel: wave j
      if (in_band && (tid >> 6) == (int)j) cls_tile_edges(mask[j], start, (uint64_t)f * T + tt, a, lane);
      if (!in_band) continue;
      const bool fast = start >= 3 * (int64_t)W + 3;
      uint32_t* recs = a.recs + (uint64_t)f * a.rec_stride + start;
      uint32_t rec[CLS_PPT];
#pragma unroll
      for (int q = 0; q < CLS_PPT; ++q) {
        const int p = q * CLS_THREADS + tid;
        const uint32_t cs = j * ENC_TILE + q * CLS_THREADS;   // strip column of thread 0
        const bool coded = (coded_bits >> (2 * j + q)) & 1u;
        const uint32_t* b0 = win[y & 3] + cs + tid;
        const uint32_t* b1 = win[(y - 1) & 3] + cs + tid;
        const uint32_t* b2 = win[(y - 2) & 3] + cs + 3 + tid;
        const uint32_t* b3 = win[(y - 3) & 3] + cs + tid;
        uint32_t rf;
        if (fast)
          rf = classify_y<false>(b0, b1, b2, b3, &win[0][0], (uint32_t)tid, W, 0u, ltab[j][q], cbr, csd, b0[3]);
        else
          rf = classify_y<true>(b0, b1, b2, b3, &win[0][0], (uint32_t)tid, W, (uint32_t)(start + p), ltab[j][q], cbr,
                                csd, b0[3]);
        rec[q] = coded ? rf : cunc;
      }
#pragma unroll
      for (int q = 0; q < CLS_PPT; ++q) {
        const int p = q * CLS_THREADS + tid;
        const bool coded = (coded_bits >> (2 * j + q)) & 1u;
        recs[p] = rec[q];
        slot_hist_add(hs, rec[q]);
        if constexpr (!MASK_OUT)   // (else enc_rundigits counts them)
          cls_run_digits(run_hist, wbal[j][q], lane, p, ENC_TILE, mask[j], coded);
      }
    }
  }
  cls_hist_flush<true, false>(a, f, hs, run_hist);   // (one frame per block: no re-zero)
}
// ---------------------------------------------------------------------------
// K1w: classify with per-tile row windows (rows too wide for any ring and not
// whole tiles per strip row: RGBA with W > CLS_RING2_MAX_W and W % 1024 != 0,
// RGB with W > CLS_RING2_MAX_W).  Each block walks a contiguous tile range
// like the ring kernels; for each tile it stages four LINEAR windows,
// window r = pixels [start - rW - 3, start - rW + 1027) in Y space, so every
// reference of the tile's pixels (0..3 rows back, 3 pixels either side,
// wrapping across row ends as code.rs:141-145's linear offsets do) is inside
// the window of its row offset.  Rows above are read from HBM/L2 once per
// window (4 B/px more than the ring's single read); the next tile's windows
// load into registers while this one is classified.  The mode decision is the
// ring kernels' classify_y over explicit window bases.
// ---------------------------------------------------------------------------
constexpr int TW_RS = ENC_TILE + 8;                                         // window words
constexpr int TW_LD = (ENC_TILE + 6 + CLS_THREADS - 1) / CLS_THREADS;       // loads per window per thread (3)

template <int C, bool MASK_OUT>
__device__ __forceinline__ void enc_classify_twin_body(const EncArgs& a) {
  __shared__ uint32_t win[4][TW_RS];
  __shared__ uint32_t hs[C0_N + 2 * SX_N];
  __shared__ uint32_t run_hist[8];
  __shared__ uint32_t mask[ENC_TILE / 32];
  __shared__ uint32_t ltab[CLS_PPT][16];
  uint64_t w_begin, w_end;
  if (!cls_work_range(a, w_begin, w_end)) return;
  const int tid = threadIdx.x, lane = tid & 63;
  uint32_t cbr, csd, cunc;
  cls_lane_consts((uint32_t)lane, cbr, csd, cunc);
  const uint32_t W = a.W;
  const int64_t N = (int64_t)W * a.H;
  cls_hist_zero(hs, run_hist);
  // luma reference k of slot q's thread 0: window lr_rows(k), column q * 512 + 3 - lr_px(k)
  if (tid < 16 * CLS_PPT) {
    const int q = tid >> 4, k = tid & 15;
    ltab[q][k] = k < 11 ? (uint32_t)(lr_rows(k) * TW_RS + q * CLS_THREADS + 3 - lr_px(k)) : 0u;
  }
  // the tile's four windows into registers
  uint32_t pw[4][TW_LD];
  auto fetch = [&](const TileIter& ti) {
    const uint8_t* fr = a.px + (uint64_t)ti.f * a.frame_stride;
    const int64_t start = (int64_t)ti.tt() * ENC_TILE;
    const int64_t lo = max((int64_t)0, a.px_lo), hi = min(N, a.px_hi);
#pragma unroll
    for (int r = 0; r < 4; ++r) cls_window_load<C>(pw[r], fr, start - (int64_t)r * W - 3, ENC_TILE + 6, lo, hi);
  };
  TileIter it(a, w_begin), nx(a, w_begin);
  uint32_t cur_frame = it.f;
  fetch(nx);
  nx.step(1);
  for (uint64_t w = w_begin; w < w_end; ++w, it.step(1)) {
    const uint32_t f = it.f;
    if (f != cur_frame) {
      cls_hist_flush(a, cur_frame, hs, run_hist);
      cur_frame = f;
    }
    const int64_t start = (int64_t)it.tt() * ENC_TILE;
    const int count = (int)min((int64_t)ENC_TILE, N - start);
    __syncthreads();   // the previous tile's readers are done with the windows
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int k = 0; k < TW_LD; ++k) {
        const int c = tid + k * CLS_THREADS;
        if (c < ENC_TILE + 6) win[r][c] = y_from_rgba(pw[r][k]);
      }
    if (w + 1 < w_end) fetch(nx);
    nx.step(1);
    __syncthreads();
    // (no s_setprio(0) here, unlike ring / pair / slide: a scheduling change, wants an A/B of its own)
    // coded flags -> tile bitmask (a pixel is coded iff i == 0 or Y(i) != Y(i-1))
    uint32_t coded_bits = 0;
    unsigned long long wbal[CLS_PPT];
#pragma unroll
    for (int q = 0; q < CLS_PPT; ++q) {
      const int p = q * CLS_THREADS + tid;
      const int64_t i = start + p;
      const bool coded = p < count && (i == 0 || win[0][p + 3] != win[0][p + 2]);
      wbal[q] = __ballot(coded);
      cls_flags_out<MASK_OUT>(wbal[q], mask, a, it.tile(), q, tid, lane);
      coded_bits |= (coded ? 1u : 0u) << q;
    }
    __syncthreads();
    if (tid < 64) cls_tile_edges(mask, start, it.tile(), a, tid);   // first / last coded pixel of the tile
    const bool fast = start >= 3 * (int64_t)W + 3;
    uint32_t* recs = a.recs + (uint64_t)f * a.rec_stride + start;
    uint32_t rec[CLS_PPT];
#pragma unroll
    for (int q = 0; q < CLS_PPT; ++q) {
      const int p = q * CLS_THREADS + tid;
      const bool coded = (coded_bits >> q) & 1u;
      const uint32_t* b0 = &win[0][p];
      const uint32_t* b1 = &win[1][p];
      const uint32_t* b2 = &win[2][p + 3];
      const uint32_t* b3 = &win[3][p];
      uint32_t rf;
      if (fast)   // block-uniform
        rf = classify_y<false>(b0, b1, b2, b3, &win[0][0], (uint32_t)tid, W, 0u, ltab[q], cbr, csd, b0[3]);
      else
        rf = classify_y<true>(b0, b1, b2, b3, &win[0][0], (uint32_t)tid, W, (uint32_t)(start + p), nullptr, cbr,
                              csd, b0[3]);
      rec[q] = coded ? rf : cunc;
    }
#pragma unroll
    for (int q = 0; q < CLS_PPT; ++q) {
      const int p = q * CLS_THREADS + tid;
      const bool coded = (coded_bits >> q) & 1u;
      if (p < count) recs[p] = rec[q];
      slot_hist_add(hs, rec[q]);
      if constexpr (!MASK_OUT)   // (else enc_rundigits counts them)
        cls_run_digits(run_hist, wbal[q], lane, p, count, mask, coded);
    }
  }
  cls_hist_flush(a, cur_frame, hs, run_hist);
}
__global__ __launch_bounds__(CLS_THREADS) void enc_classify_twin(EncArgs a) { enc_classify_twin_body<4, false>(a); }
__global__ __launch_bounds__(CLS_THREADS) void enc_classify_twin_m(EncArgs a) { enc_classify_twin_body<4, true>(a); }
__global__ __launch_bounds__(CLS_THREADS) void enc_classify_twin3(EncArgs a) { enc_classify_twin_body<3, false>(a); }
__global__ __launch_bounds__(CLS_THREADS) void enc_classify_twin3_m(EncArgs a) { enc_classify_twin_body<3, true>(a); }

__global__ __launch_bounds__(CLS_THREADS) void enc_classify_strip(EncArgs a) { enc_classify_strip_body<false>(a); }
// frames: the tiles' coded flags out, run digits by enc_rundigits
__global__ __launch_bounds__(CLS_THREADS) void enc_classify_strip_m(EncArgs a) { enc_classify_strip_body<true>(a); }

}  // namespace nice
