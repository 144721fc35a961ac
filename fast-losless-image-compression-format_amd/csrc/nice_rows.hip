// nice_rows.hip -- MI355X (gfx950) row reconstruction of the NICE2 decoder: the
// per-pixel records of nice_decode.hip (nice_dec_rec.hpp) -> pixels.
//   dec_reconstruct  one wave per frame, rows in order, one lane per row segment:
//                    segments start from an unknown entry tracked as per-channel
//                    cyclic intervals (exact once they collapse -- the predictors
//                    average with the known row above), then unconverged prefixes
//                    are recomputed exactly in rounds once their left neighbour
//                    segment is final.
//   dec_rows, dec_rows_wide, dec_rows8   one block per frame, a barrier per
//                    phase (D5b); dec_rows_flow: rows in flight inside a block
//                    (D5d); dec_rows_split: several blocks per frame (D5c).
// The multi-wave kernels differ in how their waves synchronise and in their
// pre-passes; the stages they share (record loads, class tables, W_CUR
// words, tails, the raster store) are the rows_* functions of D5b, and the
// arithmetic is nice_rows.hpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nice.h"
#include "nice_dec_rec.hpp"
#include "nice_kernels.h"
#include "nice_rows.hpp"
#include "nice_rows_body.hpp"

namespace nice {

// ---------------------------------------------------------------------------
// D5: reconstruction.
// ---------------------------------------------------------------------------
struct RecLds {
  uint32_t y4tail[4];
  int32_t ref_k[16], ref_d[16];
  int32_t ref_off32[16];   // k*W + d per record class, clamped to [0, 4] (only 0..3 are special)
  int32_t err;
  uint32_t pad[3];
};

// (spread pixels and the intervals IvS: nice_rows.hpp)
// (unspread3_perm, the D5b stages rows_* and dec_rows_body: nice_rows_body.hpp)

// Row storage: R rows x W spread pixels (R = 4 for W >= 3, else 8) and the last
// 3 pixels of row y-4 (offsets 3W+1, 3W+3).
struct RowCtx {
  uint32_t* ring;
  const uint32_t* y4tail;
  uint32_t W, y, rmask;
  __device__ __forceinline__ uint32_t* row(uint32_t r) const { return ring + (size_t)(r & rmask) * W; }
};

// Pixels [x0, x_stop) of the current row from their records; r0..r2 are the
// pixels before x0 (intervals).  Branch-free step: the averaging value and the
// reference value are both formed and one is selected.  Every value is written
// to the row (unknown ones are rewritten by the fix-up pass before anything
// reads them: the only same-row reads are of pixels 0..2, which lane 0 -- exact
// from the start -- writes at its steps 0..2, before the last segment reaches
// its last three columns; the host keeps that segment >= 6 pixels long).
// Returns the last segment-local index left unknown (-1: none).
__device__ __forceinline__ int run_segment(const RowCtx& rc, const RecLds& L, const uint32_t* recs,
                                           uint32_t x0, uint32_t x_stop, IvS r0, IvS r1, IvS r2) {
  int last_unknown = -1;
  const uint32_t y = rc.y;
  const uint32_t W = rc.W;
  uint32_t* row = rc.row(y);
  const uint32_t* up = rc.row(y - 1);       // unused on row 0
  const bool has_up = y > 0;
  for (uint32_t x = x0; x < x_stop; ++x) {
    const uint32_t r = recs[x];
    const uint32_t u = up[x];
    const bool ref = rec_cls(r) != 0;   // run pixels are class 1 (the pixel before) with c = 0
    const uint32_t c = rec_c(r);
    // reference value (kind REF): recent pixels or a pixel of the ring
    const int id = (int)rec_cls(r);
    const int off = (int)L.ref_off32[id];
    int jx = (int)x - L.ref_d[id];
    int jy = (int)y - L.ref_k[id];
    if (W >= 4) {                 // one wrap at most (|d| <= 3)
      const int wrapl = jx < 0, wrapr = jx >= (int)W;
      jx += wrapl ? (int)W : (wrapr ? -(int)W : 0);
      jy += wrapr - wrapl;
    } else {                      // tiny widths: general linear index
      const int64_t j = (int64_t)y * W + x - ((int64_t)L.ref_k[id] * W + L.ref_d[id]);
      const int64_t jj = j < 0 ? 0 : j;
      jy = (int)(jj / W);
      jx = (int)(jj - (int64_t)jy * W);
    }
    jx = min(max(jx, 0), (int)W - 1);
    const uint32_t far = (jy + 4 == (int)y && rc.rmask == 3u)
                             ? rc.y4tail[max(jx - (int)(W - 3), 0)]
                             : rc.ring[(size_t)((uint32_t)jy & rc.rmask) * W + (uint32_t)jx];
    IvS src;
    src.lo = off == 1 ? r0.lo : off == 2 ? r1.lo : off == 3 ? r2.lo : off == 0 ? 0u : far;
    src.len = off == 1 ? r0.len : off == 2 ? r1.len : off == 3 ? r2.len : 0u;
    src = ref ? src : r0;
    const IvS va = ivs_avg(r0, u, c);
    const IvS vr = ivs_add(src, c);
    const bool avg = !ref && has_up;
    const IvS v{avg ? va.lo : vr.lo, avg ? va.len : vr.len};
    row[x] = v.lo;
    last_unknown = v.len ? (int)(x - x0) : last_unknown;
    r2 = r1; r1 = r0; r0 = v;
  }
  return last_unknown;
}

// The row ring lives in LDS when it fits (LDS_ROWS) -- the address space must
// be static: a runtime LDS-or-global pointer compiles to flat_* accesses, and
// every flat access waits for all outstanding global loads.
template <bool LDS_ROWS>
__device__ __forceinline__ void dec_reconstruct_body(const DecArgs& a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  RecLds& L = *reinterpret_cast<RecLds*>(smem);
  const uint32_t W = a.W, H = a.H;
  const uint32_t R = W >= 3 ? 4u : 8u;
  const uint32_t kw = (W + 31) / 32;
  static_assert(sizeof(RecLds) <= 512, "host LDS sizing assumes RecLds <= 512 B");
  uint32_t* recbuf = reinterpret_cast<uint32_t*>(smem + 512) + ((kw + 3) & ~3u);   // row records
  uint32_t* ring;
  if constexpr (LDS_ROWS) ring = recbuf + ((W + 3) & ~3u);
  else ring = a.rowbuf + (uint64_t)blockIdx.x * R * W;
  const uint32_t f = blockIdx.x;
  const int lane = threadIdx.x;
  if (a.redo && a.hand_abort[f] != SPLIT_REDO) return;
  if (a.status[f] != 0) return;
  if (lane < 16) {
    L.ref_k[lane] = cls_rows(lane);
    L.ref_d[lane] = cls_px(lane);
    const int64_t off = (int64_t)cls_rows(lane) * W + cls_px(lane);
    L.ref_off32[lane] = (int32_t)(off < 0 ? 4 : off > 4 ? 4 : off);
  }
  if (lane == 0) L.err = 0;
  __syncthreads();
  const uint32_t S = a.seg, nseg = a.nseg;
  const uint32_t* recs = a.recs + (uint64_t)f * a.rec_stride;
  uint8_t* outp = a.px_out + (uint64_t)f * a.px_stride;
  const uint32_t OC = a.out_channels;
  const uint8_t alpha = (a.flags & NICE_DEC_ALPHA_FILL_FF) ? 255 : 0;
  const bool active = (uint32_t)lane < nseg;
  const uint32_t x0 = lane * S;
  const uint32_t x1 = active ? ((uint32_t)lane == nseg - 1 ? W : x0 + S) : x0;
  const uint32_t seglen = x1 - x0;

  unsigned long long t_a = 0, t_b = 0, t_c = 0, t_d = 0;
  for (uint32_t y = 0; y < H; ++y) {
    const unsigned long long c0 = a.stats ? __builtin_amdgcn_s_memtime() : 0;
    RowCtx rc{ring, L.y4tail, W, y, R - 1};
    if (R == 4 && y >= 4 && lane < 3) L.y4tail[lane] = rc.row(y)[W - 3 + lane];
    // this row's records, coalesced
    const uint32_t* rrow = recs + (uint64_t)y * W;
    for (uint32_t x = lane; x < W; x += 64) recbuf[x] = rec_canon(rrow[x], a.rec_tag);
    __syncthreads();
    auto linear_px = [&](int64_t j) -> uint32_t {
      if (j < 0) return 0u;   // pixel 0's left neighbour is itself, not yet written (0)
      const uint64_t jy = (uint64_t)j / W, jx = (uint64_t)j - jy * W;
      return (R == 4 && jy + 4 == y) ? L.y4tail[jx - (W - 3)] : rc.row((uint32_t)jy)[jx];
    };
    IvS r0, r1, r2;
    if (lane == 0) {
      r0 = ivs_exact(linear_px((int64_t)y * W - 1));
      r1 = ivs_exact(linear_px((int64_t)y * W - 2));
      r2 = ivs_exact(linear_px((int64_t)y * W - 3));
    } else {
      r0 = IvS{0u, SP_K}; r1 = r0; r2 = r0;
    }
    const unsigned long long c1 = a.stats ? __builtin_amdgcn_s_memtime() : 0;
    // speculative pass: lane 0 starts exact, the others from an unknown entry
    int last_unknown = -1;
    if (active) last_unknown = run_segment(rc, L, recbuf, x0, x1, r0, r1, r2);
    // fix-up rounds: an unconverged segment is recomputed exactly as soon as the
    // three pixels before it are exact (left segment converged before its last
    // three pixels, or already fixed) -- normally all in one parallel round
    unsigned long long fin = __ballot(!active || last_unknown < 0);
    unsigned long long tail_ok = __ballot(!active || last_unknown < 0 ||
                                          (seglen >= 3 && last_unknown < (int)seglen - 3));
    if (a.stats && lane == 0) {
      atomicAdd(&a.stats[0], 1ull);
      atomicAdd(&a.stats[1], (unsigned long long)__popcll(~fin));
      atomicAdd(&a.stats[2], (unsigned long long)__popcll(~tail_ok));
    }
    if (a.stats && active && last_unknown >= 0) atomicAdd(&a.stats[3], (unsigned long long)(last_unknown + 1));
    __syncthreads();
    const unsigned long long c2 = a.stats ? __builtin_amdgcn_s_memtime() : 0;
    while (fin != ~0ull) {
      const bool mine = !((fin >> lane) & 1ull);
      const bool left_ok = lane == 0 || (((fin | tail_ok) >> (lane - 1)) & 1ull);
      const bool ready = mine && left_ok;
      if (ready) {
        r0 = ivs_exact(linear_px((int64_t)y * W + x0 - 1));
        r1 = ivs_exact(linear_px((int64_t)y * W + x0 - 2));
        r2 = ivs_exact(linear_px((int64_t)y * W + x0 - 3));
        const int lu = run_segment(rc, L, recbuf, x0, x0 + (uint32_t)last_unknown + 1, r0, r1, r2);
        if (lu >= 0) atomicCAS(&L.err, 0, NICE_E_FORMAT);   // exact inputs give exact outputs
        last_unknown = -1;
      }
      __syncthreads();
      fin |= __ballot(ready);
      tail_ok |= fin;
      if (a.stats && lane == 0) atomicAdd(&a.stats[4], 1ull);
    }
    __syncthreads();
    const unsigned long long c3 = a.stats ? __builtin_amdgcn_s_memtime() : 0;
    if (L.err) break;
    // emit the row in the caller's pixel format
    uint8_t* orow = outp + (uint64_t)y * W * OC;
    const uint32_t* row = rc.row(y);
    if (OC == 4) {
      uint32_t* o32 = reinterpret_cast<uint32_t*>(orow);
      for (uint32_t x = lane; x < W; x += 64) o32[x] = unspread3(row[x]) | ((uint32_t)alpha << 24);
    } else {
      for (uint32_t x = lane; x < W; x += 64) {
        const uint32_t v = unspread3(row[x]);
        uint8_t* o = orow + (uint64_t)x * 3;
        o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16);
      }
    }
    __syncthreads();
    if (a.stats) {
      const unsigned long long c4 = __builtin_amdgcn_s_memtime();
      t_a += c1 - c0; t_b += c2 - c1; t_c += c3 - c2; t_d += c4 - c3;
    }
  }
  if (a.stats && lane == 0) {
    atomicAdd(&a.stats[5], t_a); atomicAdd(&a.stats[6], t_b);
    atomicAdd(&a.stats[7], t_c); atomicAdd(&a.stats[8], t_d);
  }
  if (lane == 0 && L.err) set_status(&a.status[f], L.err);
}

// Ring in LDS (4 rows fit next to the block's tails) or in global memory.
__global__ __launch_bounds__(ROWS_THREADS) void dec_rows(DecArgs a) { dec_rows_body<ROWS_THREADS, true>(a); }
__global__ __launch_bounds__(ROWS_WIDE_THREADS) void dec_rows_wide(DecArgs a) { dec_rows_body<ROWS_WIDE_THREADS, false>(a); }
// 8-pixel segments (W <= 4096: up to 512 lanes): twice the lanes per frame,
// for batches too small to fill the CUs (single-frame latency)
__global__ __launch_bounds__(ROWS_THREADS) void dec_rows8(DecArgs a) { dec_rows_body<ROWS_THREADS, true, 8>(a); }

// ---------------------------------------------------------------------------
// D5d: dataflow row reconstruction for small batches (round 5; 64 <= W <=
// 4096, one frame per block, frames <= CUs).  dec_rows keeps every wave of a
// block on one row: a block barrier after the speculative pass, two per fix-up
// round, one after the emit, and the record pre-pass and the raster stores on
// the row's critical path.  At one frame per CU (single frames, config 3,
// small RGB batches) that path sets the decode time: 2160 rows of ~6.8 us for
// 4K.  Here the block's waves form K groups of WPR = ceil(segments / 64)
// waves; group g reconstructs rows g, g + K, ..., so rows overlap, and the
// waves synchronise only through LDS stamps (row + 1):
//   fin[slot][w]  wave w's segments of the row are final in the ring;
//   tst[slot][w]  the last three pixels of wave w's last segment are exact
//                 (tail[slot][w]): the next wave's first lane can fix up;
//   hst[slot]     the row's first three pixels (W_CUR references of the
//                 row's last columns, code.rs:141-145: offsets W-1, W-3 reach
//                 into the current row).
// Wave w of row y waits for row y-1's waves w-1..w+1 (the references reach
// +-3 pixels, rows 1..3 back: rows y-2, y-3 are final by induction), wave 0
// for all of row y-1 (its entry is the row's last pixels, code.rs:412-413),
// the last wave also for row y-1's wave 0 (right halos).  Then: pre-pass ring
// reads (the record decode and addresses are done before the wait), the
// speculative pass, and fix-up rounds inside the wave (lane shuffles, no
// barriers; the first lane takes the left wave's published tail), the ring
// row and halos, the stamp, and only then the raster stores and the next
// rows' record loads -- off the critical path.  A ring of 8 rows (K + 3 <= 8)
// in LDS.  Every dependency points to an earlier (row, wave) and all waves
// are resident, so the earliest unfinished one always progresses; every wait
// is bounded (0.2 s, then the frame fails with NICE_E_HIP and the other waves
// stop).
// ---------------------------------------------------------------------------
// (FLOW_THREADS, FLOW_SLOTS, FLOW_MAXW and struct FlowCtl: nice_geom.h)
constexpr unsigned long long FLOW_TIMEOUT = 20000000ull;   // s_memrealtime ticks (100 MHz): 0.2 s
// a timed-out wait (the workgroup preempted or time-sliced for longer than
// that) does not fail the frame: it is marked for the barrier kernel
// (dec_rows, launched after this one in redo mode) -- slower,
// never wrong
constexpr int FLOW_REDO = 1;
static_assert(sizeof(FlowPair) == sizeof(uint2) && alignof(FlowPair) == alignof(uint2), "FlowCtl::rtab");
__device__ __forceinline__ uint32_t flow_peek(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// LDS-only release (the raster stores and record loads stay in flight)
__device__ __forceinline__ void flow_publish(uint32_t* p, uint32_t v) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void flow_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local"); }
// the wave waits until stamps[i] >= want for every bit i of mask (lanes 0..3
// read one stamp each); false when the frame aborted or the wait timed out
__device__ __forceinline__ bool flow_wait(FlowCtl& C, const uint32_t* stamps, uint32_t mask, uint32_t want) {
  const uint32_t lane = threadIdx.x & 63u;
  const bool mine = lane < FLOW_MAXW && ((mask >> lane) & 1u);
  unsigned long long t0 = 0;
  for (uint32_t n = 0;; ++n) {
    const uint32_t v = mine ? flow_peek(stamps + lane) : want;
    if (__ballot(v < want) == 0ull) break;
    if ((n & 31u) == 0u) {
      if (flow_peek(&C.abort)) return false;
      const unsigned long long t = __builtin_amdgcn_s_memrealtime();
      if (n == 0) t0 = t;
      else if (t - t0 > FLOW_TIMEOUT) {
        atomicOr(&C.abort, 1u);
        atomicCAS(&C.err, 0, FLOW_REDO);
        return false;
      }
    }
    __builtin_amdgcn_s_sleep(1);
  }
  flow_acquire();
  return true;
}
// lane l gets lane l-1's value (lane 0: 0) by a DPP wave shift: one VALU move,
// no LDS round trip (ds_bpermute) on the hand-off path (one 4K frame 10.27 ->
// 10.21 ms, 64 x 1080p 4.79 -> 4.74, profiles/r05zl_ab_flow_dpp.log)
__device__ __forceinline__ uint32_t shfl_up1(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}
// The speculative pass; reports which parts of the segment stayed unknown
// (from OR trees over the interval widths instead of a compare and select per
// pixel): any pixel, any of pixels 8..15 (the fix-up chain's second half),
// any of the last three (the tail the next lane or wave starts from).  (A vote
// after pixel 7 switching the wave to the exact step when every lane's last
// three pixels were exact was neutral: 18.73 vs 18.64 ms at 512 frames,
// profiles/r05w_ab_flow_spec.log.)
struct SpecUnk { uint32_t any, hi, tail; };
template <int S, bool CUR>
__device__ __forceinline__ SpecUnk rows_spec_unk(IvS (&v)[S], IvS r0, IvS r1, IvS r2, const uint32_t (&w)[S],
                                                 const uint32_t (&prev)[S]) {
  static_assert(S == 16, "halves of eight pixels");
#pragma unroll
  for (int p = 0; p < S; ++p) {
    const IvS l1 = p >= 1 ? v[p - 1] : r0;
    const IvS l2 = p >= 2 ? v[p - 2] : (p == 1 ? r0 : r1);
    const IvS l3 = p >= 3 ? v[p - 3] : (p == 2 ? r0 : (p == 1 ? r1 : r2));
    v[p] = rows_step<CUR>(l1, l2, l3, prev[p], w[p]);
  }
  const uint32_t tail = v[13].len | v[14].len | v[15].len;
  const uint32_t hi = tail | v[8].len | v[9].len | v[10].len | v[11].len | v[12].len;
  const uint32_t lo = v[0].len | v[1].len | v[2].len | v[3].len | v[4].len | v[5].len | v[6].len | v[7].len;
  return SpecUnk{lo | hi, hi, tail};
}
// Exact recompute of pixels 0..7 and, when some lane with `hi` goes, 8..15,
// of the lanes with `go` (their entry is exact); the second half
// only when some lane of the wave still has unknown pixels there (one vote per
// round: 512 x 4K reconstruct -1 %, 1024 x 1080p -2 %, profiles/r05v_ab_chunks.log;
// votes every four pixels cost more than they saved at one frame per CU).
template <int S>
__device__ __forceinline__ void rows_chain_upto(IvS (&v)[S], IvS r0, IvS r1, IvS r2, const uint32_t (&w)[S],
                                                const uint32_t (&prev)[S], bool go, bool hi) {
  auto step = [&](int p) {
    const uint32_t l1 = p >= 1 ? v[p - 1].lo : r0.lo;
    const uint32_t l2 = p >= 2 ? v[p - 2].lo : (p == 1 ? r0.lo : r1.lo);
    const uint32_t l3 = p >= 3 ? v[p - 3].lo : (p == 2 ? r0.lo : (p == 1 ? r1.lo : r2.lo));
    const uint32_t n = rows_step_exact(l1, l2, l3, prev[p], w[p]);
    // a lane with an exact entry recomputes every pixel of the half (the ones
    // past its last unknown come out equal): one select on a lane mask per
    // pixel instead of a compare and a select (with the caller's asm pin of
    // the words, which cost a copy of each per round, removed: 512 x 4K
    // reconstruct 17.53 -> 16.86 ms, one 4K frame 9.56 -> 9.08,
    // profiles/r05zq_ab_flow_chain.log)
    v[p].lo = go ? n : v[p].lo;
  };
#pragma unroll
  for (int p = 0; p < 8; ++p) step(p);
  if (__ballot(go && hi) != 0ull) {
#pragma unroll
    for (int p = 8; p < 16; ++p) step(p);
  }
}
__global__ __launch_bounds__(FLOW_THREADS) void dec_rows_flow(DecArgs a) {
  constexpr int S = ROWS_SEG;
  extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
  FlowCtl& C = *reinterpret_cast<FlowCtl*>(sm);
  constexpr uint32_t CTL_WORDS = sizeof(FlowCtl) / 4;
  constexpr uint32_t ZERO_IDX = offsetof(FlowCtl, zero) / 4;
  const uint32_t W = a.W, H = a.H, f = blockIdx.x;
  const uint32_t RS = rows_ring_stride(W);
  const uint32_t RB = CTL_WORDS + ROWS_RB;   // sm index of ring slot 0, pixel 0
  const uint32_t RM = a.flow_ring - 1u;      // ring rows - 1 (4 or 8 rows)
  uint32_t* const ring = sm + RB;
  for (uint32_t i = threadIdx.x; i < CTL_WORDS; i += blockDim.x) sm[i] = 0u;
  __syncthreads();
  if (a.status[f] != 0) return;   // block-uniform
  const uint32_t nseg = (W + S - 1) / S, WPR = (nseg + 63) / 64, K = a.flow_k;
  const uint32_t wid = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (wid >= K * WPR) return;   // no barrier below this point
  // tests (NICE_OPT_TEST_FLOW_ABSENT): the block's last wave never starts, as
  // if it were not resident, so the others' waits time out into the fallback
  if (a.test_absent_strip && wid == K * WPR - 1) return;
  const uint32_t g = wid / WPR, w = wid - g * WPR, lastw = WPR - 1;
  const uint32_t seg = w * 64u + lane;
  const bool active = seg < nseg;
  const uint32_t x0 = seg * S;
  const int nvalid = active ? (int)min((uint32_t)S, W - x0) : 0;
  const uint32_t* recs = a.recs + (uint64_t)f * a.rec_stride;
  uint8_t* outp = a.px_out + (uint64_t)f * a.px_stride;
  const uint32_t OC = a.out_channels;
  const uint32_t alpha = (a.flags & NICE_DEC_ALPHA_FILL_FF) ? 0xFF000000u : 0u;
  const uint32_t asel = alpha ? 0x0D060100u : 0x0C060100u;   // unspread3_perm
  const bool vec_rec = (W & 3u) == 0 && nvalid == S;
  const bool vec_out = (OC == 4 && (W & 3u) == 0 && nvalid == S) ||
                       (OC == 3 && (W & 15u) == 0 && nvalid == S);
  const uint32_t full = (1u << WPR) - 1u;
  const uint32_t depmask = w == 0 ? full : ((((7u << w) >> 1) & full) | (w == lastw ? 1u : 0u));
  const bool curlane = active && x0 + S + 2u >= W;   // words that can reference row y itself (W_CUR)
  const bool wave_cur = __any(curlane);
  uint2* const rtab = reinterpret_cast<uint2*>(C.rtab[wid]);
  const uint32_t lb = 17u * seg;
  uint32_t rn[S];
  auto load_recs = [&](uint32_t y) { rows_load_recs<S>(rn, recs + (uint64_t)y * W + x0, vec_rec, nvalid); };
  if (g < H) load_recs(g);
  bool ok = true;
#ifdef NICE_FLOW_STATS   // cycle split per wave position (NICE_DEC_STATS=1): stats[64 + 8 w + k]
  unsigned long long ts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define FLOW_T(k) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); ts[k] += t_ - tlast; tlast = t_; }
  unsigned long long tlast = __builtin_amdgcn_s_memtime();
#else
#define FLOW_T(k)
#endif
  for (uint32_t y = g; y < H && ok; y += K) {
    const uint32_t s = y & (FLOW_SLOTS - 1u);                              // stamps
    const uint32_t rs = y & RM, rsp = (y - 1u) & RM;   // ring rows
    // ---- pre-pass, part 1 (no pixel values): the row's class table, each
    // record's constant and kind bits, and the ring index of its reference
    if (lane < 16) rtab[lane] = rows_tab_entry(lane, y, RM, RS, RB);   // its .y: an sm index
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    uint32_t wk[S], ad[S];
#pragma unroll
    for (int p = 0; p < S; ++p) {
      const uint32_t r = rec_canon(rn[p], a.rec_tag);
      const uint32_t cls = rec_cls(r);   // 0..13
      const uint2 e = rtab[cls];
      uint32_t idx = lb + e.y + (uint32_t)p;
      if (p < 3 || p > S - 4) idx += (uint32_t)((int)(p + 3u - (e.x & 7u)) >> 4);   // padding word crossed
      ad[p] = cls >= 4u ? idx : ZERO_IDX;
      // kind bits | the constant (already spread by the writers): one bit-field
      // insert (e.x holds only kind bits 28..31 and dxp3 in bits 0..2, which
      // the constant's mask covers)
      uint32_t kw;
      asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(kw) : "s"(REC_K), "v"(r), "v"(e.x));
      wk[p] = kw;
    }
    // references past the row end into row y itself (pixels 0..2): only the
    // wave holding the row's last columns (a wave-uniform branch: as a lane
    // branch the compiler if-converted it into every wave's pre-pass once the
    // record constant no longer needed spreading here, +2 % reconstruct)
    if (wave_cur) {
#pragma unroll
      for (int p = 0; p < S; ++p) {
        wk[p] = rows_cur_word(wk[p], rn[p], a.rec_tag, x0 + p, W, curlane);
        ad[p] = (wk[p] & W_CUR) ? ZERO_IDX : ad[p];   // (no word has that bit before: e.x has no bit 18)
      }
    }
    FLOW_T(0)
    // ---- wait for the rows above
    if (y > 0 && !flow_wait(C, C.fin[(y - 1u) & (FLOW_SLOTS - 1u)], depmask, y)) { ok = false; break; }
    // wave priorities (round 6): the row's pass once the rows above are in
    // before the waves still decoding records or storing the raster, and the
    // fix-up chain -- the row's serial path -- before both (512 x 4K
    // reconstruct 15.54 -> 14.48 ms, one 4K frame 8.43 -> 7.92;
    // profiles/r06ze_ab_flow_prio.log, r06zf_ab_flow_prio2.log)
    __builtin_amdgcn_s_setprio(1);
    FLOW_T(1)
    // ---- pre-pass, part 2: reference values, the row above, the entry
    uint32_t wv[S], prev[S];
#pragma unroll
    for (int p = 0; p < S; ++p) {
      const uint32_t o = sm[ad[p]];
      wv[p] = (wk[p] & ~SP_K) | ((o + wk[p]) & SP_K);
    }
    uint32_t* const pr = ring + rsp * RS;
#pragma unroll
    for (int p = 0; p < S; ++p) prev[p] = y > 0 ? pr[lb + p] : 0u;
    IvS r0{0u, SP_K}, r1{0u, SP_K}, r2{0u, SP_K};
    if (seg == 0) {
      if (y == 0) {
        r0 = r1 = r2 = ivs_exact(0u);
      } else {
        r0 = rows_entry_prev(pr, W, 1); r1 = rows_entry_prev(pr, W, 2); r2 = rows_entry_prev(pr, W, 3);
      }
    }
    FLOW_T(2)
    // ---- speculative pass
    IvS v[S];
    // (a wave without the row's last columns skips the W_CUR width term:
    // 512 x 4K reconstruct -1 %, profiles/r05zt_ab_flow_curspec.log)
    const SpecUnk su = wave_cur ? rows_spec_unk<S, true>(v, r0, r1, r2, wv, prev)
                                : rows_spec_unk<S, false>(v, r0, r1, r2, wv, prev);
    bool fin = !active || su.any == 0u;
    bool tex = !active || su.tail == 0u;
    const bool unk_hi = su.hi != 0u;
    if (w == 0 && lane == 0) {   // the row's first three pixels (lane 0: exact entry)
      C.head[s][0] = v[0].lo; C.head[s][1] = v[1].lo; C.head[s][2] = v[2].lo;
      flow_publish(&C.hst[s], y + 1u);
    }
    bool tpub = w == lastw;   // the last wave's tail feeds no wave
    auto pub_tail = [&]() {
      if (!tpub && __builtin_amdgcn_readlane((int)tex, 63)) {
        if (lane == 63) {
          C.tail[s][w][0] = v[S - 1].lo; C.tail[s][w][1] = v[S - 2].lo; C.tail[s][w][2] = v[S - 3].lo;
          flow_publish(&C.tst[s][w], y + 1u);
        }
        tpub = true;
      }
    };
    pub_tail();
    FLOW_T(3)
    // ---- fix-up rounds inside the wave
    __builtin_amdgcn_s_setprio(2);
    bool cur_done = !wave_cur;
    unsigned long long t0 = 0;
    for (uint32_t n = 0;; ++n) {
      if (__ballot(!fin) == 0ull) break;
      if (!cur_done && flow_peek(&C.hst[s]) >= y + 1u) {
        flow_acquire();
        const uint32_t h0 = C.head[s][0], h1 = C.head[s][1], h2 = C.head[s][2];
        if (curlane) rows_resolve_cur<S>(wv, h0, h1, h2);
        cur_done = true;
      }
      IvS l0{shfl_up1(v[S - 1].lo), 0u}, l1{shfl_up1(v[S - 2].lo), 0u}, l2{shfl_up1(v[S - 3].lo), 0u};
      bool lex = shfl_up1(tex ? 1u : 0u) != 0u;
      if (lane == 0) {
        lex = false;
        if (w > 0 && flow_peek(&C.tst[s][w - 1]) >= y + 1u) {
          flow_acquire();
          l0.lo = C.tail[s][w - 1][0]; l1.lo = C.tail[s][w - 1][1]; l2.lo = C.tail[s][w - 1][2];
          lex = true;
        }
      }
      const bool go = !fin && lex && (cur_done || !curlane);
      if (__ballot(go) != 0ull) {
        rows_chain_upto<S>(v, l0, l1, l2, wv, prev, go, unk_hi);
        if (go) {
          fin = true;
          tex = true;
        }
        pub_tail();
#ifdef NICE_FLOW_STATS
        ts[6] += 1;
#endif
      } else {
        // nothing to do until the left wave's tail or the row head arrive
        if ((n & 31u) == 0u) {
          if (flow_peek(&C.abort)) { ok = false; break; }
          const unsigned long long t = __builtin_amdgcn_s_memrealtime();
          if (t0 == 0) t0 = t;
          else if (t - t0 > FLOW_TIMEOUT) {
            atomicOr(&C.abort, 1u);
            atomicCAS(&C.err, 0, FLOW_REDO);
            ok = false;
            break;
          }
        }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    FLOW_T(4)
    if (!ok) break;
    if (C.err) { atomicOr(&C.abort, 1u); ok = false; break; }
    // ---- the ring row, its halos, the stamp
    if (active) {
      uint32_t* rr = ring + rs * RS + lb;
#pragma unroll
      for (int p = 0; p < S; ++p) rr[p] = v[p].lo;   // padding pixels land in the row's spare words
      // row y-1's right halo: this row's first three pixels (row 0: ring row
      // -1's, which row 2's last columns read, as in dec_rows)
      if (seg == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) pr[(W + k) + ((W + k) >> 4)] = v[k].lo;
      }
    }
    if (wave_cur) {   // row y+1's left halo (words -4..-2): this row's columns W-3..W-1, copied
      // from the ring words just written by the wave holding each of them
      // (a 4-row ring puts it over row y-3's left halo, which row y's first
      // wave reads in its pre-pass: wait for that wave's first pixels)
      if (RM < 7u && !flow_wait(C, &C.hst[s], 1u, y + 1u)) { ok = false; break; }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
      const uint32_t col = W - 3u + lane;
      if (lane < 3u && (col / S) / 64u == w)
        ring[((y + 1u) & RM) * RS + lane - 4] = ring[rs * RS + col + (col >> 4)];
    }
    if (lane == 0) flow_publish(&C.fin[s][w], y + 1u);
    __builtin_amdgcn_s_setprio(0);
    FLOW_T(5)
    // ---- off the critical path: the next row's records, the raster
    if (y + K < H) load_recs(y + K);
    if (active) rows_store_raster<S>(outp, (uint64_t)y * W + x0, v, OC, vec_out, nvalid, alpha, asel);
  }
  if (lane == 0) {
    const int e = __hip_atomic_load(&C.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (e == FLOW_REDO && a.hand_abort) atomicCAS(&a.hand_abort[f], 0u, SPLIT_REDO);
    else if (e) set_status(&a.status[f], e == FLOW_REDO ? NICE_E_HIP : e);
  }
#ifdef NICE_FLOW_STATS
  if (lane == 0 && a.stats) {
    // ts[7]: rows processed; k = 0 record decode, 1 wait, 2 ring reads, 3 spec, 4 fix-up, 5 ring row + stamp, 6 fix-up rounds with work
    ts[7] = (H > g ? (H - g + K - 1) / K : 0);
    for (int k = 0; k < 8; ++k) atomicAdd(&a.stats[64 + 8 * w + k], ts[k]);
  }
#endif
#undef FLOW_T
}

// ---------------------------------------------------------------------------
// D5c: strip-split reconstruction for wide frames: a frame's row segments are
// cut into k strips of <= 256 lanes, one workgroup each (one per CU), all rows
// in order.  In raster order the strip-rows ("units" (y, j)) form one chain:
// a unit's left neighbour is (y, j-1), or (y-1, k-1) for j = 0 (the wrap of
// code.rs:412-413), its right neighbour (y, j+1), or (y+1, 0).  Each block
// keeps a 4-row ring of its columns plus three halo columns on each side in
// LDS; ring row r's left halo is the last three pixels of r's left neighbour
// unit, its right halo the first three of r's right neighbour unit -- so every
// reference (rows 1..3 back, +-3 pixels, code.rs:141-145) is one ring read
// with no wrap logic, and lane 0's entry (the three pixels before the strip)
// is ring row y's left halo.  Units publish their first and last three pixels
// as soon as they are exact (after the speculative pass, usually without
// their entry) as 8-byte {row + 1, value} granules (agent-scope relaxed
// atomics: sc1 stores / loads); a block waits for nothing before its
// speculative pass except the halos of rows y-2 and y-3 (published long
// before); halo words of row y-1 not yet published and the entry are unknown
// intervals in the speculative pass, resolved in the fix-up rounds, which poll
// for them.  Every dependency points to a unit earlier in raster order, so
// with every block resident (the host launches at most one block per CU for
// half the CUs) the earliest unfinished unit always progresses.  Polls give up
// after SPLIT_TIMEOUT (a frame-wide abort flag stops the other strips early
// on an error).
// ---------------------------------------------------------------------------
// (SPLIT_THREADS, SPLIT_GRAN, split_ring_stride and the LDS layout: nice_geom.h)
// s_memrealtime ticks (100 MHz): 0.2 s.  A wait this long means a strip's
// neighbour is not resident (other kernels hold the CUs): the frame is handed
// to the fallback launch (SPLIT_REDO), not failed
constexpr unsigned long long SPLIT_TIMEOUT = 20000000ull;
constexpr int SPLIT_QUIET = -1000, SPLIT_TIMED_OUT = -1001;   // block-local err codes
__device__ __forceinline__ uint32_t sr_idx(uint32_t lc3) { return lc3 + (lc3 >> 4); }

__device__ __forceinline__ void hand_put(unsigned long long* p, uint32_t row, uint32_t v) {
  __hip_atomic_store(p, ((unsigned long long)(row + 1u) << 32) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long hand_get(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct SplitGeo {
  uint32_t f, j, k, W, H, sw, RS;
  unsigned long long* hand;   // frame f's granules
  // granule i of unit (y, jj)
  __device__ __forceinline__ unsigned long long* g(uint32_t y, uint32_t jj, uint32_t i) const {
    return hand + ((uint64_t)y * k + jj) * SPLIT_GRAN + i;
  }
  // source granule of halo pixel i (0..2) of ring row r (>= -1: ring row -1's
  // right halo is row 0's first pixels when j = k-1 -- pixel W-3 of row 0
  // may reference pixel 0 through offset W-3), side 0 (left) / 1 (right);
  // false when the source lies outside the image (never referenced)
  __device__ __forceinline__ bool src(int r, uint32_t side, uint32_t i, unsigned long long*& p,
                                      uint32_t& srow) const {
    if (side == 0) {
      if (j > 0) {
        if (r < 0) return false;
        p = g((uint32_t)r, j - 1, 4 + i); srow = (uint32_t)r; return true;
      }
      if (r < 1) return false;
      p = g((uint32_t)r - 1, k - 1, 4 + i); srow = (uint32_t)r - 1; return true;
    }
    if (j + 1 < k) {
      if (r < 0) return false;
      p = g((uint32_t)r, j + 1, i); srow = (uint32_t)r; return true;
    }
    if (r < -1 || r + 1 >= (int)H) return false;
    p = g((uint32_t)(r + 1), 0, i); srow = (uint32_t)(r + 1); return true;
  }
};

// A wave-0 poll in two halves, so the granule loads' latency overlaps other
// work.  The halo items of row y: t = 0..5 ring rows y-3, y-3, y-2, y-2, y-1,
// y-1 (left, right), t = 6 row y's left halo (the entry); lanes 3t..3t+2 take
// item t.  issue() loads the granules of the items in `mask` whose hv word
// does not say present; commit() copies every item whose three tags match
// into the ring and sets its hv word.  hv[slot * 2 + side]: the ring row
// (>= -1) whose halo the slot holds, + 2 (0: none).
struct HaloPoll {
  unsigned long long v;
  int r;
  uint32_t side, i, srow;   // side 2: no item on this lane
  bool ex;
  __device__ __forceinline__ void issue(const SplitGeo& G, const uint32_t* hv, uint32_t lane, uint32_t y,
                                        uint32_t mask) {
    side = 2u;
    ex = false;
    v = 0;
    const uint32_t t = lane / 3u;
    i = lane - 3u * t;
    if (t >= 7u || !((mask >> t) & 1u)) return;
    const int rr = t < 6u ? (int)y - 3 + (int)(t >> 1) : (int)y;
    const uint32_t sd = t < 6u ? (t & 1u) : 0u;
    if (rr < -1 || hv[((uint32_t)rr & 3u) * 2u + sd] == (uint32_t)(rr + 2)) return;
    r = rr;
    side = sd;
    unsigned long long* p = nullptr;
    ex = G.src(rr, sd, i, p, srow);
    if (ex) v = hand_get(p);
  }
  __device__ __forceinline__ void commit(const SplitGeo& G, uint32_t* ring, uint32_t* hv, uint32_t lane) {
    const bool ok = side < 2u && (!ex || (uint32_t)(v >> 32) == srow + 1u);
    if (ok) ring[((uint32_t)r & 3u) * G.RS + sr_idx(side ? G.sw + 3u + i : i)] = (uint32_t)v;
    const unsigned long long m = __ballot(ok);
    if (ok && i == 0u && ((m >> lane) & 7ull) == 7ull) hv[((uint32_t)r & 3u) * 2u + side] = (uint32_t)(r + 2);
    side = 2u;
  }
};
// present bits (t = 0..6) of row y's halo items
__device__ __forceinline__ uint32_t halo_have(const uint32_t* hv, uint32_t y) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t t = 0; t < 7u; ++t) {
    const int rr = t < 6u ? (int)y - 3 + (int)(t >> 1) : (int)y;
    const uint32_t sd = t < 6u ? (t & 1u) : 0u;
    if (rr < -1 || hv[((uint32_t)rr & 3u) * 2u + sd] == (uint32_t)(rr + 2)) m |= 1u << t;
  }
  return m;
}

__global__ __launch_bounds__(SPLIT_THREADS) void dec_rows_split(DecArgs a) {
  constexpr int S = ROWS_SEG;
  extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
  __shared__ uint32_t clsw[32];
  __shared__ uint32_t hv[8];     // ring slot halo state (row + 1 per slot and side)
  __shared__ uint32_t pend[2];
  __shared__ int err;
  const uint32_t k = a.strips;
  const uint32_t f = a.split_f0 + blockIdx.x / k, j = blockIdx.x % k;
  if (a.test_absent_strip && j == k - 1) return;   // block-uniform (tests only)
  const uint32_t W = a.W, H = a.H;
  const uint32_t nseg = (W + S - 1) / S;
  const uint32_t sps = (nseg + k - 1) / k;
  const uint32_t s0 = j * sps, s1 = min(nseg, s0 + sps);
  const uint32_t c0 = s0 * S, sw = min(W, s1 * S) - c0;
  const uint32_t lane = threadIdx.x;
  const uint32_t nl = s1 - s0;
  const bool active = lane < nl;
  const uint32_t xl0 = lane * S;
  const int nvalid = active ? (int)min((uint32_t)S, sw - xl0) : 0;
  const SplitGeo G{f, j, k, W, H, sw, split_ring_stride(sw), a.hand + (uint64_t)f * H * k * SPLIT_GRAN};
  const uint32_t RS = G.RS;
  uint32_t* tails = sm;                              // SPLIT_THREADS x {lo, len} x 3
  uint32_t* flags = sm + SPLIT_FLAGS;                // SPLIT_THREADS
  uint32_t* ring = sm + SPLIT_RING;                  // 4 x RS
  rows_fill_clsw(clsw);
  if (threadIdx.x < 8) hv[threadIdx.x] = 0;
  if (lane == 0) err = 0;
  if (a.status[f] != 0) return;   // block-uniform
  uint32_t* abort_f = a.hand_abort + f;
  const uint32_t* recs = a.recs + (uint64_t)f * a.rec_stride + c0;
  uint8_t* outp = a.px_out + (uint64_t)f * a.px_stride;
  const uint32_t OC = a.out_channels;
  const uint32_t alpha = (a.flags & NICE_DEC_ALPHA_FILL_FF) ? 0xFF000000u : 0u;
  const uint32_t asel = alpha ? 0x0D060100u : 0x0C060100u;   // unspread3_perm
  const bool vec_rec = ((W | c0) & 3u) == 0 && nvalid == S;
  const bool vec_out = (OC == 4 && ((W | c0) & 3u) == 0 && nvalid == S) ||
                       (OC == 3 && ((W | c0) & 15u) == 0 && nvalid == S);
  uint32_t prev[S], rn[S];
#pragma unroll
  for (int p = 0; p < S; ++p) prev[p] = 0;
  auto load_recs = [&](uint32_t y) { rows_load_recs<S>(rn, recs + (uint64_t)y * W + xl0, vec_rec, nvalid); };
  if (H > 0) load_recs(0);
  __syncthreads();
  unsigned long long t_row = 0;   // when this row's waits began
  // wave 0: gives up (error) on a timeout or another strip's abort
  auto give_up = [&]() -> bool {
    if (__hip_atomic_load(abort_f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
      if (lane == 0) atomicCAS(&err, 0, SPLIT_QUIET);   // another strip failed or timed out: exit quietly
      return true;
    }
    if (__builtin_amdgcn_s_memrealtime() - t_row > SPLIT_TIMEOUT) {
      if (lane == 0) atomicCAS(&err, 0, SPLIT_TIMED_OUT);
      return true;
    }
    return false;
  };
  HaloPoll HP;
  bool pending_poll = false;   // wave 0: HP holds issued loads
  // timing counters (NICE_DEC_STATS=1) only in -DNICE_ROWS_STATS builds
#ifdef NICE_ROWS_STATS
  unsigned long long* const stats = a.stats;
#else
  constexpr unsigned long long* stats = nullptr;
#endif
  unsigned long long c_entry = 0, c_right = 0;
  unsigned long long c_wait = 0, c_spec = 0, c_fix = 0, c_emit = 0, n_rounds = 0, n_polls = 0, n_noentry = 0;
  uint32_t y = 0;
  for (; y < H; ++y) {
    const unsigned long long cc0 = stats ? __builtin_amdgcn_s_memtime() : 0;
    // ---- halos: rows y-2 and y-3 (wait), row y-1 and the entry (try)
    t_row = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) {   // slot y & 3 held row y-4: free it for row y
      hv[(y & 3u) * 2u] = 0u;
      hv[(y & 3u) * 2u + 1u] = 0u;
    }
    if (lane < 64) {
      // the loads issued at the end of the previous row, then rows y-2 and
      // y-3 (items 0..3) until present
      if (pending_poll) HP.commit(G, ring, hv, lane);
      pending_poll = false;
      while (true) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
        const uint32_t miss = ~halo_have(hv, y) & 15u;
        if (!miss) break;
        if (give_up()) break;
        HP.issue(G, hv, lane, y, miss);
        HP.commit(G, ring, hv, lane);
        if (stats) ++n_polls;
        __builtin_amdgcn_s_sleep(1);
      }
    }
    __syncthreads();
    if (err) break;
    const uint32_t ym1 = (y - 1u) & 3u;
    bool hl1 = hv[ym1 * 2u] == y + 1u;               // row y-1's halos present (row -1 at y = 0)
    bool hr1 = hv[ym1 * 2u + 1u] == y + 1u;
    bool eok = hv[(y & 3u) * 2u] == y + 2u;          // the entry (row y's left halo)
    const unsigned long long cc1 = stats ? __builtin_amdgcn_s_memtime() : 0;
    if (stats && !eok) ++n_noentry;
    // ---- pre-pass: records -> per-pixel words; a reference into a halo of
    // row y-1 not yet present is marked W_CUR (unknown) with its halo slot
    // (index in bits 8..9, side in bit 19) and resolved in the fix-up rounds
    const uint32_t* const cwt = clsw + (y == 0 ? 16 : 0);
    uint32_t w[S];
    bool npend = false;
#pragma unroll
    for (int p = 0; p < S; ++p) {
      const uint32_t r = rec_canon(rn[p], a.rec_tag);
      const uint32_t cls = rec_cls(r);
      const uint32_t cw = cwt[cls];
      const uint32_t rows = cw & 3u;
      const uint32_t lc3 = xl0 + (uint32_t)p + 6u - ((cw >> 2) & 7u);   // local column + 3 - pixels back
      const bool up = cls >= 4;
      const bool pl = up && rows == 1u && lc3 < 3u && !hl1;
      const bool pr = up && rows == 1u && lc3 >= sw + 3u && !hr1;
      const uint32_t lcc = min(lc3, sw + 5u);
      const uint32_t o = ring[__umul24((y - rows) & 3u, RS) + sr_idx(lcc)];
      const uint32_t c = rec_c(r);
      const bool cur = pl || pr;
      const uint32_t hslot = pl ? lc3 : (lc3 - sw - 3u);
      const uint32_t kb = (cw & 0xF0000000u) | (cur ? W_CUR : 0u);
      w[p] = kb | ((up && !cur) ? ((o + c) & SP_K) : c) | (cur ? ((hslot << 8) | (pr ? (1u << 19) : 0u)) : 0u);
      npend = npend || cur;
    }
    // ---- entry: exact when present (strip 0 of row 0: zeros), else unknown
    IvS r0{0u, SP_K}, r1{0u, SP_K}, r2{0u, SP_K};
    if (lane == 0) {
      if (y == 0 && j == 0) {
        r0 = r1 = r2 = ivs_exact(0u);
      } else if (eok) {
        const uint32_t* hr = ring + (y & 3u) * RS;
        r0 = ivs_exact(hr[sr_idx(2)]); r1 = ivs_exact(hr[sr_idx(1)]); r2 = ivs_exact(hr[sr_idx(0)]);
      }
    }
    if (y + 1 < H) load_recs(y + 1);
    // ---- speculative pass
    IvS v[S];
    int lu = rows_spec<S>(v, r0, r1, r2, w, prev);
    if (active) {
      rows_put_tail<S>(tails + lane * 6, v);
      flags[lane] = (lu < S - 3) ? 1u : 0u;
    }
    if (lane == 0) { pend[0] = 0; pend[1] = 0; }
    bool fin = !active || lu < 0;
    // the unit's first / last three pixels, published once exact
    uint32_t pub = 0;
    const bool pub_lane = active && (lane == 0 || xl0 + S + 3u > sw);
    auto publish = [&]() {
      if (!pub_lane) return;
#pragma unroll
      for (int p = 0; p < S; ++p) {
        const uint32_t x = xl0 + (uint32_t)p;
        const uint32_t il = x + 3u - sw;   // 0..2 for the last three pixels
        if (x < 3u && !((pub >> x) & 1u) && v[p].len == 0u) {
          hand_put(G.g(y, j, x), y, v[p].lo);
          pub |= 1u << x;
        }
        if (x < sw && il < 3u && !((pub >> (4u + il)) & 1u) && v[p].len == 0u) {
          hand_put(G.g(y, j, 4u + il), y, v[p].lo);
          pub |= 16u << il;
        }
      }
    };
    publish();
    rows_barrier<true>();
    const unsigned long long cc2 = stats ? __builtin_amdgcn_s_memtime() : 0;
    // ---- fix-up rounds (polling for the entry and row y-1's missing halos)
    for (uint32_t rd = 0;; ++rd) {
      if (stats) ++n_rounds;
      if (!fin) atomicOr(&pend[rd & 1u], 1u);
      if (lane < 64) {
        // commit the loads issued last round, issue the still missing items
        // (row y-1's halos, the entry); their latency overlaps this round
        if (pending_poll) HP.commit(G, ring, hv, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
        const uint32_t miss = ~halo_have(hv, y) & 0x70u;
        pending_poll = miss != 0u;
        if (pending_poll) {
          HP.issue(G, hv, lane, y, miss);
          if (stats) ++n_polls;
          if (rd > 1u) __builtin_amdgcn_s_sleep(1);
        }
      }
      if (lane < 64 && (rd & 63u) == 63u) (void)give_up();   // bounds every wait (and any logic error)
      rows_barrier<true>();
      if (pend[rd & 1u] == 0 || err) break;
      if (lane == 0) pend[(rd + 1) & 1u] = 0;
      const bool nhl = hl1 || hv[ym1 * 2u] == y + 1u, nhr = hr1 || hv[ym1 * 2u + 1u] == y + 1u;
      if (npend && ((nhl && !hl1) || (nhr && !hr1))) {
        // halo words now present: resolve them (their chains are unknown from
        // there on and get recomputed below)
        const uint32_t* hrow = ring + ym1 * RS;
        bool still = false;
#pragma unroll
        for (int p = 0; p < S; ++p) {
          if (w[p] & W_CUR) {
            const uint32_t sd = (w[p] >> 19) & 1u, hs = (w[p] >> 8) & 3u;
            if (sd ? nhr : nhl)
              w[p] = (hrow[sr_idx(sd ? sw + 3u + hs : hs)] + (w[p] & SP_K)) & SP_K;
            else
              still = true;
          }
        }
        npend = still;
      }
      hl1 = nhl;
      hr1 = nhr;
      const bool neok = eok || hv[(y & 3u) * 2u] == y + 2u;
      if (stats && neok && !eok) c_entry += __builtin_amdgcn_s_memtime() - cc2;
      if (stats && nhr && !hr1) c_right += __builtin_amdgcn_s_memtime() - cc2;
      eok = neok;
      bool exact_in = false;
      bool go = !fin;
      if (!fin) {
        if (lane > 0) {
          rows_get_tail(tails + (lane - 1) * 6, r0, r1, r2);
          exact_in = flags[lane - 1] != 0;
        } else if (eok) {
          const uint32_t* hr = ring + (y & 3u) * RS;
          r0 = ivs_exact(hr[sr_idx(2)]); r1 = ivs_exact(hr[sr_idx(1)]); r2 = ivs_exact(hr[sr_idx(0)]);
          exact_in = true;
        }
        exact_in = exact_in && !npend;
        // as in dec_rows: only exact left tails (or entries) are used
        go = exact_in;
      }
      rows_barrier<true>();
      lu = rows_chain_exact<S>(v, r0, r1, r2, w, prev, lu, go);
      if (go) {
        if (lu >= 0) atomicCAS(&err, 0, NICE_E_FORMAT);
        rows_put_tail<S>(tails + lane * 6, v);
        flags[lane] = 1u;
        fin = true;
      }
      publish();
    }
    if (err) break;
    // prefetch the next row's halo items (committed at its start)
    if (lane < 64 && y + 1 < H) {
      if (pending_poll) HP.commit(G, ring, hv, lane);
      HP.issue(G, hv, lane, y + 1, 0x7Fu);
      pending_poll = true;
    }
    const unsigned long long cc3 = stats ? __builtin_amdgcn_s_memtime() : 0;
    // ---- emit: ring row y (local columns) and the raster
    if (active) {
      uint32_t* rr = ring + (y & 3u) * RS;
      const uint64_t pix = (uint64_t)y * W + c0 + xl0;
#pragma unroll
      for (int p = 0; p < S; ++p) rr[sr_idx(xl0 + (uint32_t)p + 3u)] = v[p].lo;   // padding: spare words
      rows_store_raster<S>(outp, pix, v, OC, vec_out, nvalid, alpha, asel);
    }
#pragma unroll
    for (int p = 0; p < S; ++p) prev[p] = v[p].lo;
    rows_barrier<true>();
    if (stats) {
      const unsigned long long cc4 = __builtin_amdgcn_s_memtime();
      c_wait += cc1 - cc0; c_spec += cc2 - cc1; c_fix += cc3 - cc2; c_emit += cc4 - cc3;
    }
  }
  if (stats && lane == 0) {
    atomicAdd(&stats[0], (unsigned long long)y); atomicAdd(&stats[4], n_rounds);
    atomicAdd(&stats[5], c_wait); atomicAdd(&stats[6], c_spec); atomicAdd(&stats[7], c_fix);
    atomicAdd(&stats[8], c_emit); atomicAdd(&stats[1], n_noentry); atomicAdd(&stats[2], n_polls);
    atomicAdd(&stats[3], c_entry); atomicAdd(&stats[9], c_right);
  }
  if (lane == 0 && err) {
    if (err == SPLIT_TIMED_OUT) {
      // not co-resident: the fallback launch reconstructs the frame (a real
      // error of another strip sets the status, which the fallback respects)
      atomicCAS(abort_f, 0u, SPLIT_REDO);
    } else if (err != SPLIT_QUIET) {
      __hip_atomic_store(abort_f, SPLIT_ABORT_ERR, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      set_status(&a.status[f], err);
    }
  }
}

__global__ __launch_bounds__(64) void dec_reconstruct(DecArgs a) {
  if (a.rows_in_lds) dec_reconstruct_body<true>(a);
  else dec_reconstruct_body<false>(a);
}

}  // namespace nice
