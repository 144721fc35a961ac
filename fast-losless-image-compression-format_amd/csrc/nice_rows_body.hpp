// nice_rows_body.hpp -- the barrier row kernels' body (dec_rows, dec_rows8,
// dec_rows_wide: nice_rows.hip) and the rows_* stages it shares with
// dec_rows_flow and dec_rows_split.  The device compiles this text; a plain
// C++ compiler reads it too, through the HIP names of tools/hip_host_shim, so
// tools/rows_host_check.cpp (tests/test_rows_host.py) runs the same statements
// on host threads under sanitizers, every buffer at its planned size.  What
// needs wave intrinsics, spin-waits or inline ISA stays in nice_rows.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nice.h"
#include "nice_dec_rec.hpp"
#include "nice_kernels.h"
#include "nice_rows.hpp"

// The two spots a host compiler cannot read as the device does: the dynamic
// LDS declaration (host: the shim's block buffer) and the opaque register
// barrier ("+v" is a VGPR constraint).
#if defined(__HIPCC__)
#define NICE_ROWS_DYN_LDS(name) extern __shared__ __attribute__((aligned(16))) uint32_t name[]
#define NICE_ROWS_OPAQUE(x) asm volatile("" : "+v"(x))
#else
#define NICE_ROWS_DYN_LDS(name) uint32_t* const name = static_cast<uint32_t*>(hip_host_shim::dyn_lds)
#define NICE_ROWS_OPAQUE(x) asm volatile("" : "+r"(x))
#endif

namespace nice {

// unspread3(v) | alpha by two byte permutes of v (R), v >> 2 (G), v >> 4 (B):
// asel = 0x0D060100 (alpha byte 0xFF) or 0x0C060100 (0x00); 4 instructions
// per pixel instead of 7
__device__ __forceinline__ uint32_t unspread3_perm(uint32_t v, uint32_t asel) {
  const uint32_t rg = __builtin_amdgcn_perm(v >> 2, v, 0x0C0C0500u);
  return __builtin_amdgcn_perm(v >> 4, rg, asel);
}

// ---------------------------------------------------------------------------
// D5b: multi-wave reconstruction (64 <= W <= 16384).  One block per frame,
// one lane per 16-pixel row segment (up to 1024 lanes).  A lane keeps its
// segment of the row above and of the current row in registers (the segment
// loop is unrolled), so the left-to-right recurrence touches no memory:
//   pre-pass  records (prefetched one row ahead) -> per-pixel kind and
//             constant; references into rows above read a ring of the last
//             four rows (LDS when it fits, else global)
//   spec      from the exact entry (lane 0) or an unknown one (others), as
//             per-channel cyclic intervals that collapse within a few pixels
//   fix-up    rounds across the block: a lane whose left neighbour's last
//             three pixels are exact recomputes its unknown prefix exactly;
//             the others refine theirs from the neighbour's current intervals
//             (sound, so anything that collapses is final)
//   emit      pixels to the ring and the caller's raster
// ---------------------------------------------------------------------------
// (ROWS_SEG, ROWS_RING and the kernels' LDS layouts: nice_geom.h; the per-pixel
// word, its kinds and the one-pixel steps rows_step / rows_step_exact:
// nice_rows.hpp)

// Speculative pass over the whole segment; returns -1 when every pixel is
// exact, S - 4 when the last three are, else S - 1 (a bound on the last unknown).
// (Switching a wave to the plain step once all its lanes are exact -- one
// vote per pixel -- was 5 % slower: each vote's branch waits on the VALU.)
// A partial last segment's padding pixels are run records (copies of the pixel
// before, interval width included), so counting them leaves "every pixel
// exact" unchanged and spares 16 loop-invariant lane masks (SGPR spills).
template <int S>
__device__ __forceinline__ int rows_spec(IvS (&v)[S], IvS r0, IvS r1, IvS r2, const uint32_t (&w)[S],
                                         const uint32_t (&prev)[S]) {
#pragma unroll
  for (int p = 0; p < S; ++p) {
    const IvS l1 = p >= 1 ? v[p - 1] : r0;
    const IvS l2 = p >= 2 ? v[p - 2] : (p == 1 ? r0 : r1);
    const IvS l3 = p >= 3 ? v[p - 3] : (p == 2 ? r0 : (p == 1 ? r1 : r2));
    v[p] = rows_step(l1, l2, l3, prev[p], w[p]);
  }
  // a coarse last unknown index from two OR trees instead of a compare and a
  // select per pixel: its users only ask "any unknown" and "last three exact",
  // and the fix-up chain recomputing exact pixels too is harmless (512-frame
  // reconstruct 20.03 -> 19.63 ms)
  uint32_t head = 0, tail = v[S - 1].len | v[S - 2].len | v[S - 3].len;
#pragma unroll
  for (int p = 0; p < S - 3; ++p) head |= v[p].len;
  return tail ? S - 1 : head ? S - 4 : -1;
}

// Recomputes pixels 0..lu (lanes with `go`), keeping the others (already
// exact); returns the new last unknown index.  Stops once no lane of the wave
// has work left.
template <int S>
__device__ __forceinline__ int rows_chain(IvS (&v)[S], IvS r0, IvS r1, IvS r2, const uint32_t (&w)[S],
                                          const uint32_t (&prev)[S], int lu, bool go) {
  int nlu = -1;
  const int upto = go ? lu : -1;
#pragma unroll
  for (int p = 0; p < S; ++p) {
    if (!__any(p <= upto)) break;
    const IvS l1 = p >= 1 ? v[p - 1] : r0;
    const IvS l2 = p >= 2 ? v[p - 2] : (p == 1 ? r0 : r1);
    const IvS l3 = p >= 3 ? v[p - 3] : (p == 2 ? r0 : (p == 1 ? r1 : r2));
    const IvS n = rows_step(l1, l2, l3, prev[p], w[p]);
    const bool upd = p <= upto;
    v[p].lo = upd ? n.lo : v[p].lo;
    v[p].len = upd ? n.len : v[p].len;
    nlu = (upd && n.len) ? p : nlu;
  }
  return go ? nlu : lu;
}

template <int S>
__device__ __forceinline__ int rows_chain_exact(IvS (&v)[S], IvS r0, IvS r1, IvS r2, const uint32_t (&w)[S],
                                                const uint32_t (&prev)[S], int lu, bool go) {
  const int upto = go ? lu : -1;
  // all S steps, predicated: a vote per pixel to stop early (its branch waits
  // on the VALU) made a single 4K frame 4 % slower, same at 512 frames (one
  // vote per call to skip waves with nothing to recompute, and kind masks
  // instead of the select chain, were no faster either)
#pragma unroll
  for (int p = 0; p < S; ++p) {
    const uint32_t l1 = p >= 1 ? v[p - 1].lo : r0.lo;
    const uint32_t l2 = p >= 2 ? v[p - 2].lo : (p == 1 ? r0.lo : r1.lo);
    const uint32_t l3 = p >= 3 ? v[p - 3].lo : (p == 2 ? r0.lo : (p == 1 ? r1.lo : r2.lo));
    const uint32_t n = rows_step_exact(l1, l2, l3, prev[p], w[p]);
    const bool upd = p <= upto;
    v[p].lo = upd ? n : v[p].lo;
    v[p].len = upd ? 0u : v[p].len;
  }
  return go ? -1 : lu;
}

// Block barrier; with the ring in LDS only LDS traffic is ordered, so global
// stores (the raster) and the record prefetch stay in flight across it.
template <bool LDS_RING>
__device__ __forceinline__ void rows_barrier() {
  if constexpr (LDS_RING) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
  } else {
    __syncthreads();
  }
}

// ---- stages shared by dec_rows*, dec_rows_flow and dec_rows_split -----------

// One row's records of a lane's segment (rrow: its first record) into rn.
// vec: the segment is whole and 16-byte aligned.
template <int S>
__device__ __forceinline__ void rows_load_recs(uint32_t (&rn)[S], const uint32_t* rrow, bool vec, int nvalid) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < S / 4; ++q) {
      const uint4 t = reinterpret_cast<const uint4*>(rrow)[q];
      rn[4 * q] = t.x; rn[4 * q + 1] = t.y; rn[4 * q + 2] = t.z; rn[4 * q + 3] = t.w;
    }
  } else if (nvalid > 0) {   // a partial last segment
#pragma unroll
    for (int p = 0; p < S; ++p) rn[p] = p < nvalid ? rrow[p] : REC_RUN;
  } else {                   // idle lane: no loads (its wave would run the masked path every row)
#pragma unroll
    for (int p = 0; p < S; ++p) rn[p] = REC_RUN;
  }
}

// Static class word: rows back (bits 0-1), pixels back + 3 (bits 2-4), kind
// bits (28-31); y0: the kinds of row 0.
__device__ __forceinline__ uint32_t rows_cls_word(uint32_t c, bool y0) {
  const unsigned long long kinds = y0 ? ROWS_KIND_Y0 : ROWS_KIND;
  return ((CLS_ROWS_PACK >> (2 * c)) & 3u) | (uint32_t)((CLS_PX_PACK >> (3 * c)) & 7u) << 2 |
         ((uint32_t)(kinds >> (4u * c)) & 15u) << 28;
}
// The block's table of them: entries 16.. for row 0.  One LDS read per pixel
// instead of three shifts of packed 64-bit constants.
__device__ __forceinline__ void rows_fill_clsw(uint32_t (&clsw)[32]) {
  if (threadIdx.x < 32) clsw[threadIdx.x] = rows_cls_word(threadIdx.x & 15u, threadIdx.x >= 16);
}

// Per-row class-table entry (16-pixel segments) of class c on row y: x = kind
// bits | pixels back + 3, y = word (from `base`) of the referenced row's pixel
// 0 plus 3 minus pixels back, so a reference's word is 17 * lane + p + y (+ a
// +-1 padding correction for the first and last three pixels of a segment).
// With base >= ROWS_RB (the left halo words) no such sum is negative: as
// unsigned 32-bit arithmetic a negative one wraps, which an LDS address
// forgives and a 64-bit global address does not (lane 0, classes 1..3 and
// 10..12 at columns 0..2 with the referenced row in ring slot 0)
__device__ __forceinline__ uint2 rows_tab_entry(uint32_t c, uint32_t y, uint32_t ring_mask, uint32_t RS,
                                                uint32_t base) {
  const unsigned long long kinds = y == 0 ? ROWS_KIND_Y0 : ROWS_KIND;
  const uint32_t rows = (CLS_ROWS_PACK >> (2 * c)) & 3u, dxp3 = (uint32_t)(CLS_PX_PACK >> (3 * c)) & 7u;
  return make_uint2((((uint32_t)(kinds >> (4u * c)) & 15u) << 28) | dxp3,
                    base + ((y - rows) & ring_mask) * RS + 3u - dxp3);
}

// A reference past the row end into row y itself (pixels 0..2; only columns
// W-3 .. W-1 have them): the word w of column x becomes W_CUR | constant |
// pixel index in bits 8..9.  Branch-free (per-pixel branches held exec masks
// in SGPRs, which spilled); lane_ok masks lanes of the calling wave that hold
// no such column.  By value and per pixel, the loop in the callers: as one
// function over the segment's arrays dec_rows_wide spilled 12 more registers
// (and a second function for "is it one" did not fold into this one: 5 more).
__device__ __forceinline__ uint32_t rows_cur_word(uint32_t w, uint32_t rec, uint32_t tag, uint32_t x, uint32_t W,
                                                  bool lane_ok) {
  const uint32_t r = rec_canon(rec, tag);   // padding: a run record (class 1)
  const uint32_t cls = rec_cls(r);
  const uint32_t tx = x + 3u - ((uint32_t)(CLS_PX_PACK >> (3u * cls)) & 7u);
  const bool cur = lane_ok && cls >= 4u && ((CLS_ROWS_PACK >> (2u * cls)) & 3u) == 1u && tx >= W;
  return cur ? (W_CUR | rec_c(r) | ((tx - W) << 8)) : w;
}
// ... and once the row's pixels 0..2 (h0..h2) are exact, plain constants
template <int S>
__device__ __forceinline__ void rows_resolve_cur(uint32_t (&w)[S], uint32_t h0, uint32_t h1, uint32_t h2) {
#pragma unroll
  for (int p = 0; p < S; ++p) {
    const uint32_t k = (w[p] >> 8) & 3u;
    const uint32_t hv = k == 0u ? h0 : k == 1u ? h1 : h2;
    w[p] = (w[p] & W_CUR) ? ((hv + (w[p] & SP_K)) & SP_K) : w[p];
  }
}

// A lane's tail in LDS: its last three pixels as six words {lo, len} x 3
// (pixels S-1, S-2, S-3), the entry of the lane to its right.
template <int S>
__device__ __forceinline__ void rows_put_tail(uint32_t* t, const IvS (&v)[S]) {
  t[0] = v[S - 1].lo; t[1] = v[S - 1].len;
  t[2] = v[S - 2].lo; t[3] = v[S - 2].len;
  t[4] = v[S - 3].lo; t[5] = v[S - 3].len;
}
__device__ __forceinline__ void rows_get_tail(const uint32_t* t, IvS& r0, IvS& r1, IvS& r2) {
  r0 = IvS{t[0], t[1]}; r1 = IvS{t[2], t[3]}; r2 = IvS{t[4], t[5]};
}

// Pixel k (1..3) from the end of a padded ring row pr: lane 0's entry on a row
// y > 0 is the previous row's last three pixels, exact.
__device__ __forceinline__ IvS rows_entry_prev(const uint32_t* pr, uint32_t W, uint32_t k) {
  return ivs_exact(pr[(W - k) + ((W - k) >> 4)]);
}

// A segment's pixels (pix: the raster index of its first) in the caller's
// format: OC = 4 (alpha: the fill byte << 24, asel: its unspread3_perm
// selector) or 3 bytes per pixel.  vec_out: the segment is whole and its
// bytes 16-byte aligned (RGB: whole groups of 16 pixels, 48 bytes).
template <int S>
__device__ __forceinline__ void rows_store_raster(uint8_t* outp, uint64_t pix, const IvS (&v)[S], uint32_t OC,
                                                  bool vec_out, int nvalid, uint32_t alpha, uint32_t asel) {
  if (vec_out && OC == 4) {
    uint4* o = reinterpret_cast<uint4*>(outp + pix * 4);
#pragma unroll
    for (int q = 0; q < S / 4; ++q)
      o[q] = make_uint4(unspread3_perm(v[4 * q].lo, asel), unspread3_perm(v[4 * q + 1].lo, asel),
                        unspread3_perm(v[4 * q + 2].lo, asel), unspread3_perm(v[4 * q + 3].lo, asel));
  } else if (vec_out) {
    if constexpr (S % 16 == 0) {
      uint32_t b[3 * S / 4];
#pragma unroll
      for (int q = 0; q < S / 4; ++q) {
        const uint32_t u0 = unspread3_perm(v[4 * q].lo, 0x0C060100u), u1 = unspread3_perm(v[4 * q + 1].lo, 0x0C060100u);
        const uint32_t u2 = unspread3_perm(v[4 * q + 2].lo, 0x0C060100u), u3 = unspread3_perm(v[4 * q + 3].lo, 0x0C060100u);
        b[3 * q] = __builtin_amdgcn_perm(u1, u0, 0x04020100u);       // R0 G0 B0 R1
        b[3 * q + 1] = __builtin_amdgcn_perm(u2, u1, 0x05040201u);   // G1 B1 R2 G2
        b[3 * q + 2] = __builtin_amdgcn_perm(u3, u2, 0x06050402u);   // B2 R3 G3 B3
      }
      uint4* o = reinterpret_cast<uint4*>(outp + pix * 3);
#pragma unroll
      for (int q = 0; q < 3 * S / 16; ++q) o[q] = make_uint4(b[4 * q], b[4 * q + 1], b[4 * q + 2], b[4 * q + 3]);
    }
  } else if (OC == 4) {
    uint32_t* o32 = reinterpret_cast<uint32_t*>(outp + pix * 4);
#pragma unroll
    for (int p = 0; p < S; ++p)
      if (p < nvalid) o32[p] = unspread3(v[p].lo) | alpha;
  } else {
    uint8_t* o8 = outp + pix * 3;
#pragma unroll
    for (int p = 0; p < S; ++p) {
      if (p < nvalid) {
        const uint32_t u = unspread3(v[p].lo);
        o8[3 * p] = (uint8_t)u; o8[3 * p + 1] = (uint8_t)(u >> 8); o8[3 * p + 2] = (uint8_t)(u >> 16);
      }
    }
  }
}

template <int MAXT, bool LDS_RING, int S = ROWS_SEG>
__device__ __forceinline__ void dec_rows_body(const DecArgs& a) {
  // diagnostics counters (NICE_DEC_STATS=1) only in -DNICE_ROWS_STATS builds:
  // the runtime checks alone held SGPRs and branches in the row loop
#ifdef NICE_ROWS_STATS
  unsigned long long* const stats = a.stats;
#else
  constexpr unsigned long long* stats = nullptr;
#endif
  NICE_ROWS_DYN_LDS(sm);
  __shared__ uint32_t clsw[32];   // rows_cls_word per record class
  rows_fill_clsw(clsw);
  const uint32_t nthr = blockDim.x;
  const uint32_t W = a.W, H = a.H;
  const RowsLds lds = rows_lds(nthr);
  uint32_t* tails = sm + lds.tails;   // nthr x {lo, len} x 3 (pixels S-1, S-2, S-3)
  uint32_t* flags = sm + lds.flags;   // nthr: last three pixels exact
  uint32_t* head3 = sm + lds.head3;   // pixels 0..2 of the current row
  uint32_t* pend = sm + lds.pend;     // 2 round flags
  int* err = reinterpret_cast<int*>(sm + lds.err);
  const uint32_t f = blockIdx.x;
  // ring rows padded one word per 16 pixels: lane i's segment starts at bank
  // 17i mod 32, so the lanes' accesses to their segments are conflict free
  const uint32_t RS = rows_ring_stride(W);
  uint32_t* const ring0 = LDS_RING ? (sm + lds.ring) : (a.rowbuf + (uint64_t)f * ROWS_RING * RS);
  uint32_t* ring = ring0 + ROWS_RB;   // slot 0, pixel 0
  // per-row class table (S == 16: rows_tab_entry), double-buffered by row parity
  __shared__ uint2 rtab[2][16];
  auto build_tab = [&](uint32_t yy) {
    if (threadIdx.x < 16) rtab[yy & 1u][threadIdx.x] = rows_tab_entry(threadIdx.x, yy, ROWS_RING - 1, RS, ROWS_RB);
  };
  if (S == 16) build_tab(0);
  if (a.redo && a.hand_abort[f] != SPLIT_REDO) return;   // block-uniform
  if (a.status[f] != 0) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t nseg = (W + S - 1) / S;
  const bool active = lane < nseg;
  const uint32_t x0 = lane * S;
  // the table form's word base: idle lanes (run records, nothing stored) read
  // lane 0's words, theirs would lie past the ring
  const uint32_t lb = active ? 17u * lane : 0u;
  const int nvalid = active ? (int)min((uint32_t)S, W - x0) : 0;
  const uint32_t* recs = a.recs + (uint64_t)f * a.rec_stride;
  uint8_t* outp = a.px_out + (uint64_t)f * a.px_stride;
  const uint32_t OC = a.out_channels;
  const uint32_t alpha = (a.flags & NICE_DEC_ALPHA_FILL_FF) ? 0xFF000000u : 0u;
  const uint32_t asel = alpha ? 0x0D060100u : 0x0C060100u;   // unspread3_perm
  const bool vec_rec = (W & 3u) == 0 && nvalid == S;
  const bool vec_out = (OC == 4 && (W & 3u) == 0 && nvalid == S) ||
                       (OC == 3 && S % 16 == 0 && (W & 15u) == 0 && nvalid == S);
  if (lane == 0) *err = 0;
  uint32_t prev[S], rn[S];
#pragma unroll
  for (int p = 0; p < S; ++p) prev[p] = 0;
  auto load_recs = [&](uint32_t y) { rows_load_recs<S>(rn, recs + (uint64_t)y * W + x0, vec_rec, nvalid); };
  if (H > 0) load_recs(0);
  __syncthreads();
  unsigned long long t_a = 0, t_b = 0, t_c = 0, t_d = 0, n_fix = 0;
  for (uint32_t y = 0; y < H; ++y) {
    const unsigned long long c0 = stats ? __builtin_amdgcn_s_memtime() : 0;
    // ---- pre-pass: records -> per-pixel words
    const uint32_t* const cwt = clsw + (y == 0 ? 16 : 0);
    uint32_t w[S];
    if constexpr (S == 16) {
      // table form: every lane, no wrap logic (ring halos); only the last
      // lane's references to the current row (W_CUR) are patched below
      const uint2* tb = rtab[y & 1u];
#pragma unroll
      for (int p = 0; p < S; ++p) {
        const uint32_t r = rec_canon(rn[p], a.rec_tag);
        const uint32_t cls = rec_cls(r);                     // 0..13
        const uint2 e = tb[cls];
        uint32_t ad = lb + e.y;
        if (p < 3 || p > S - 4) ad += (uint32_t)((int)(p + 3u - (e.x & 7u)) >> 4);   // padding word crossed
        const uint32_t o = ring0[ad + p];   // e.y counts from the ring's first word: never negative
        const uint32_t c = rec_c(r);
        // (a VALU mask from a table bit instead of the compare: 4 % slower)
        w[p] = (e.x & 0xF0000000u) | (((cls >= 4u ? o : 0u) + c) & SP_K);
      }
      // references into row y itself: the last segment, and the one before
      // it when the last holds fewer than three pixels (W % 16 in {1, 2});
      // only the wave holding those lanes runs it
      if (x0 + S + 2u >= W) {
#pragma unroll
        for (int p = 0; p < S; ++p) w[p] = rows_cur_word(w[p], rn[p], a.rec_tag, x0 + p, W, true);
      }
    } else {
#pragma unroll
      for (int p = 0; p < S; ++p) {
        const uint32_t x = x0 + p;
        const uint32_t r = rec_canon(rn[p], a.rec_tag);
        const uint32_t cls = rec_cls(r);                       // 0..13
        const uint32_t cw = cwt[cls];                          // rows | px + 3 << 2 | kind bits
        const uint32_t rows = cw & 3u;
        const int dx = (int)((cw >> 2) & 7u) - 3;
        int tx = (int)x - dx;
        const int wl = tx < 0, wr = tx >= (int)W;
        tx += wl ? (int)W : (wr ? -(int)W : 0);
        const uint32_t back = rows + wl - wr;                  // rows above (0: current row)
        const bool up = cls >= 4;
        const bool cur = up && back == 0;
        // unconditional LDS read (a harmless in-range address for other classes)
        const uint32_t txc = (uint32_t)min(max(tx, 0), (int)W - 1);
        const uint32_t o = ring[__umul24((y - back) & (ROWS_RING - 1), RS) + txc + (txc >> 4)];
        const uint32_t c = rec_c(r);
        // kind bits from the class (branch-free: the ternary chain compiled to two
        // nested exec-masked branches per pixel)
        const uint32_t kb = (cw & 0xF0000000u) | (cur ? W_CUR : 0u);
        w[p] = kb | ((up && !cur) ? ((o + c) & SP_K) : c) | (cur ? ((uint32_t)tx << 8) : 0u);
      }
    }
    // ---- entry: lane 0 exact (previous row's last pixels; 0 before pixel 0)
    IvS r0{0u, SP_K}, r1{0u, SP_K}, r2{0u, SP_K};
    if (lane == 0) {
      if (y == 0) {
        r0 = r1 = r2 = ivs_exact(0u);
      } else {
        const uint32_t* pr = ring + (size_t)((y - 1) & (ROWS_RING - 1)) * RS;
        r0 = rows_entry_prev(pr, W, 1); r1 = rows_entry_prev(pr, W, 2); r2 = rows_entry_prev(pr, W, 3);
      }
    }
    if (y + 1 < H) load_recs(y + 1);   // in flight during this row
    const unsigned long long c1 = stats ? __builtin_amdgcn_s_memtime() : 0;
    // ---- speculative pass
    IvS v[S];
    int lu = rows_spec<S>(v, r0, r1, r2, w, prev);
    if (active) {
      rows_put_tail<S>(tails + lane * 6, v);
      flags[lane] = (lu < S - 3) ? 1u : 0u;
    }
    if (lane == 0) { head3[0] = v[0].lo; head3[1] = v[1].lo; head3[2] = v[2].lo; pend[0] = 0; pend[1] = 0; }
    bool fin = !active || lu < 0;
    if (stats && active && lu >= 0) {
      atomicAdd(&stats[1], 1ull);
      atomicAdd(&stats[3], (unsigned long long)(lu + 1));
      if (lu >= S - 3) atomicAdd(&stats[2], 1ull);
      // unknown tails: every tail pixel a full-width interval (a copy chain
      // from the unknown entry or a current-row reference) or some narrowed one
      const uint32_t tl0 = v[S - 1].len, tl1 = v[S - 2].len, tl2 = v[S - 3].len;
      if (tl0 | tl1 | tl2) {
        const bool copies = (tl0 == 0u || tl0 == SP_K) && (tl1 == 0u || tl1 == SP_K) && (tl2 == 0u || tl2 == SP_K);
        atomicAdd(&stats[copies ? 24 : 25], 1ull);
      }
    }
    rows_barrier<LDS_RING>();
    const unsigned long long c2 = stats ? __builtin_amdgcn_s_memtime() : 0;
    const unsigned long long nfix0 = n_fix;
    // ---- fix-up rounds
    bool cur_done = false;
    for (uint32_t rd = 0;; ++rd) {
      if (!fin) atomicOr(&pend[rd & 1u], 1u);
      rows_barrier<LDS_RING>();
      if (pend[rd & 1u] == 0) break;
      ++n_fix;
      if (lane == 0) pend[(rd + 1) & 1u] = 0;
      if (!cur_done) {   // pixels 0..2 of the row are exact now (lane 0)
        // the lanes that can hold W_CUR words (above)
        if (x0 + S + 2u >= W) rows_resolve_cur<S>(w, head3[0], head3[1], head3[2]);
        cur_done = true;
      }
      bool exact_in = false;
      if (!fin && lane > 0) {
        rows_get_tail(tails + (lane - 1) * 6, r0, r1, r2);
        exact_in = flags[lane - 1] != 0;
      }
      rows_barrier<LDS_RING>();
      // only lanes whose left tail is exact recompute, with plain arithmetic:
      // refining from an inexact neighbour (interval chain) rarely collapses
      // anything in one round and forced its whole wave onto the interval
      // chain; the leftmost unfinished lane always has an exact left tail
      const bool go = !fin && exact_in;
      // the words as opaque per round: otherwise the compiler hoists the select
      // masks of all 16 pixels out of the round loop, and their SGPR pairs
      // spill to VGPR lanes (a writelane per mask per row, a readlane per use)
#pragma unroll
      for (int p = 0; p < S; ++p) NICE_ROWS_OPAQUE(w[p]);
      lu = rows_chain_exact<S>(v, r0, r1, r2, w, prev, lu, go);
      if (go) {
        if (lu >= 0) atomicCAS(err, 0, NICE_E_FORMAT);   // exact inputs give exact outputs
        rows_put_tail<S>(tails + lane * 6, v);
        flags[lane] = 1u;
        fin = true;
      }
    }
    if (stats && lane == 0) {
      const unsigned long long r = n_fix - nfix0;
      atomicAdd(&stats[9 + (r >= 6 ? 6 : r)], 1ull);
    }
    if (*err) break;
    const unsigned long long c3 = stats ? __builtin_amdgcn_s_memtime() : 0;
    // ---- emit: ring row y (its slot held row y-4, no longer referenced) and the raster
    if (active) {
      uint32_t* rr = ring + (size_t)(y & (ROWS_RING - 1)) * RS + x0 + (x0 >> 4);   // x0 = 16 * lane
      const uint64_t pix = (uint64_t)y * W + x0;
#pragma unroll
      for (int p = 0; p < S; ++p) rr[p] = v[p].lo;   // padding pixels land in the row's spare words
      // row y-1's right halo: this row's first three pixels.  Row 0 too (ring
      // row -1, the slot row 3 takes later): row 2's last three columns reach
      // pixels 0..2 through offsets 3W-3 and 3W-1, three rows back and past the
      // row end (planted-reference tests: pixel 3W-3 read a word never written)
      if (lane == 0) {
        uint32_t* h = ring + (size_t)((y - 1) & (ROWS_RING - 1)) * RS;
#pragma unroll
        for (int k = 0; k < 3; ++k) h[(W + k) + ((W + k) >> 4)] = v[k].lo;
      }
      // row y+1's left halo: this row's last three pixels -- from the last
      // segment and, when it holds fewer than three (W % 16 in {1, 2}), the one
      // before it (round 5 width sweep: W = 66, a row starting with a W+3
      // reference read a stale halo word)
      if (x0 + S + 2u >= W) {
        uint32_t* h = ring + (size_t)((y + 1) & (ROWS_RING - 1)) * RS;
#pragma unroll
        for (int p = 0; p < S; ++p)
          if (p < nvalid && x0 + p + 3u >= W) h[(int)(x0 + p - W) - 1] = v[p].lo;
      }
      rows_store_raster<S>(outp, pix, v, OC, vec_out, nvalid, alpha, asel);
    }
#pragma unroll
    for (int p = 0; p < S; ++p) { prev[p] = v[p].lo; }
    if (S == 16) build_tab(y + 1);   // the last readers of that buffer were row y-1's
    rows_barrier<LDS_RING>();
    if (stats) {
      const unsigned long long c4 = __builtin_amdgcn_s_memtime();
      t_a += c1 - c0; t_b += c2 - c1; t_c += c3 - c2; t_d += c4 - c3;
    }
  }
  if (stats && lane == 0) {
    atomicAdd(&stats[0], (unsigned long long)H);
    atomicAdd(&stats[4], n_fix);
    atomicAdd(&stats[5], t_a); atomicAdd(&stats[6], t_b);
    atomicAdd(&stats[7], t_c); atomicAdd(&stats[8], t_d);
  }
  if (lane == 0 && *err) set_status(&a.status[f], *err);
}

}  // namespace nice
