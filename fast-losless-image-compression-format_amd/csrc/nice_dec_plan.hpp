// nice_dec_plan.hpp -- what one decode call launches, decided by a pure
// function of the batch's shape and the test options: no HIP, no globals
// (tools/dec_plan_check.cpp drives it on the CPU).  nice_capi.hip only
// allocates and launches what the plan says.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "nice_format.h"
#include "nice_geom.h"

namespace nice {

struct DecShape {
  uint32_t n_frames, w, h;
  int cus;               // compute units of the device
  uint64_t max_len;      // longest stream, bytes
  uint64_t total_bits;   // data bits of all streams (behind the file and table headers)
};
// A test / A/B option (include/nice_test.h): unset, or its value.
struct DecOpt {
  bool set;
  int64_t val;
  bool on() const { return set && val != 0; }
};
struct DecOpts { DecOpt slice_bits, single_wave, seg, split, flow, no_events, ev_cap, hev_cap; };

// the row kernels (nice_test_last_dec_route reports these values)
enum DecRoute : uint32_t { DEC_R_NONE, DEC_R_RECONSTRUCT, DEC_R_ROWS, DEC_R_ROWS8, DEC_R_ROWS_WIDE, DEC_R_FLOW, DEC_R_SPLIT };
constexpr uint32_t dec_route_max_threads(DecRoute r) {   // the kernels' launch bounds
  return r == DEC_R_RECONSTRUCT ? 64 : r == DEC_R_ROWS || r == DEC_R_ROWS8 ? ROWS_THREADS
       : r == DEC_R_ROWS_WIDE ? ROWS_WIDE_THREADS : r == DEC_R_FLOW ? FLOW_THREADS : r == DEC_R_SPLIT ? SPLIT_THREADS : 0;
}
struct DecLaunch {
  DecRoute route;
  uint32_t threads;
  size_t lds;   // dynamic LDS bytes
};
// dec_reconstruct's row segments, ring rows and LDS
struct RecGeom {
  uint32_t seg, nseg, R;
  size_t lds;
  bool in_lds;
};
struct DecPlan {
  uint32_t slice_bits, max_chunks, ck_bits, n_ck, ev_cap, subs;
  uint32_t hev_cap;     // head events kept per slice by the re-parses (0: none)
  DecLaunch rows;       // the row kernel of every frame; DEC_R_NONE: rows too wide to decode
  DecLaunch fallback;   // DEC_R_NONE, or the redo launch for frames the flow / split kernel gave up on
  uint32_t strips, split_frames;   // split: strips per frame, frames per launch
  uint32_t flow_k, flow_ring;      // flow: row groups in flight, ring rows
  size_t rowbuf, hand;             // scratch bytes: row rings in global memory, the strips' hand-off granules
  bool abort_flags;                // per-frame redo flags
  RecGeom g;
};

inline RecGeom rec_geom(uint32_t w) {
  auto align4 = [](size_t v) { return (v + 3) / 4 * 4; };
  RecGeom g;
  uint32_t s = (w + DEC_MAX_SEGS - 1) / DEC_MAX_SEGS;
  if (s < 6) s = 6;
  g.seg = s;
  g.nseg = w ? (w + s - 1) / s : 1;
  // the last segment (which runs to W) must be >= 6 pixels: its last three
  // columns read pixels 0..2 of the same row, written by lane 0 at steps 0..2
  if (g.nseg > 1 && w - (g.nseg - 1) * s < 6) g.nseg -= 1;
  g.R = w >= 3 ? 4 : 8;
  const size_t kw = (w + 31) / 32;
  const size_t head = 512 + align4(kw) * 4 + align4(w) * 4;   // RecLds <= 512 B, records
  const size_t ring = (size_t)g.R * w * 4;
  g.in_lds = head + ring <= 150 * 1024;
  g.lds = g.in_lds ? head + ring : head;
  return g;
}

inline DecPlan plan_decode(const DecShape& s, const DecOpts& o) {
  const uint32_t w = s.w, n_frames = s.n_frames;
  DecPlan p{};
  const uint64_t D = FILE_HEADER_BYTES * 8 + TABLE_HEADER_BITS;
  // slice size: long slices make the Jacobi re-parses (which run until the
  // slowest lane of a wave re-synchronises, ~1000 bits) cheap relative to the
  // first pass, short ones keep a small batch filling the GPU: aim for about
  // 256 CUs x 8 waves x 64 lanes x 2 slices, as a power of two in [1K, 16K]
  // (at least 2048 bits from ~48 Mbit of streams up: a 1024-bit slice holds
  // no checkpoint, so every Jacobi re-parse and dec_emit walk whole slices --
  // one 4K frame 9.75 -> 9.61 ms, 4 x 4K 10.03 -> 9.85, 8 x 1080p 5.17 ->
  // 5.11; one 1080p frame, whose 2048-bit slices leave the GPU emptier, 4.92
  // -> 4.96: kept at 1024, profiles/r06v_ab_slice_min.log)
  uint32_t cb = s.total_bits >= (48ull << 20) ? 2 * DEC_MIN_CHUNK_BITS : DEC_MIN_CHUNK_BITS;
  while (cb < DEC_MAX_CHUNK_BITS && s.total_bits / (2ull * cb) > 256ull * 8 * 64 * 2) cb *= 2;
  if (o.slice_bits.set) {   // tests: force a slice size
    const uint32_t v = (uint32_t)o.slice_bits.val;
    if (v >= DEC_MIN_CHUNK_BITS && v <= DEC_MAX_CHUNK_BITS && (v & (v - 1)) == 0) cb = v;
  }
  p.slice_bits = cb;
  p.max_chunks = s.max_len * 8 > D ? (uint32_t)((s.max_len * 8 - D + cb - 1) / cb) : 1;
  // checkpoints every 512 bits in slices up to 4K bits (small batches: the
  // re-parses and dec_emit's heads stop at the first meeting point, half as far
  // in: one 4K frame 9.59 -> 9.52 ms, 64 x 1080p 6.13 -> 6.07), every 1024 from
  // 8K bits up (512 x 4K: sync 12.0 -> 12.6 ms at 512, more checkpoint stores
  // than the shorter heads save; profiles/r06x_ab_ck_bits.log)
  p.ck_bits = cb <= 4096u ? DEC_CK_BITS_SMALL : DEC_CK_BITS;
  p.n_ck = cb / p.ck_bits - 1;
  p.subs = cb / DEC_EMIT_BITS;
  // keep the first sync pass's pixel events (one per >= 4 bits of a slice;
  // a slice with more parses its events again in dec_emit); the caller clears
  // ev_cap when the scratch does not fit, then dec_emit parses every slice again
  p.ev_cap = o.no_events.on() ? 0u : cb / 4;
  if (o.ev_cap.set) {   // tests: force event overflow
    const uint32_t v = (uint32_t)o.ev_cap.val;
    if (p.ev_cap && v >= 4 && v % 4 == 0 && v < p.ev_cap) p.ev_cap = v;
  }
  // keep each re-parse's events as well, up to the second checkpoint (where
  // nearly every re-parse has met the previous parse; a head with more events
  // is parsed again in dec_emit); only with the first pass's events, and the
  // caller clears hev_cap first when the scratch does not fit
  {
    const uint32_t head_bits = 2 * p.ck_bits < cb ? 2 * p.ck_bits : cb;
    p.hev_cap = p.ev_cap ? (head_bits / 4 + 3u) & ~3u : 0u;
  }
  if (o.hev_cap.set) {   // tests: force head overflow
    const uint32_t v = (uint32_t)o.hev_cap.val;
    if (p.hev_cap && v >= 4 && v % 4 == 0 && v < p.hev_cap) p.hev_cap = v;
  }
  const RecGeom g = p.g = rec_geom(w);
  const uint32_t cus = (uint32_t)(s.cus > 1 ? s.cus : 1);

  // multi-wave row kernel for 64 <= W <= 16384 (one lane per 16-pixel segment),
  // single-wave kernel otherwise
  const uint32_t nseg16 = (w + ROWS_SEG - 1) / ROWS_SEG;
  const uint32_t rows_wpr = (nseg16 + 63) / 64, rows_thr = rows_wpr * 64;
  const bool single_wave = o.single_wave.on();
  const bool use_rows = w >= 64 && rows_thr <= ROWS_WIDE_THREADS && !single_wave;
  const size_t rows_lds = rows_lds_bytes(rows_thr, w, true);
  const bool rows_in_lds = rows_thr <= ROWS_THREADS && lds_fits(rows_lds);
  // 8-pixel segments (twice the lanes per frame) only on request
  // (NICE_DEC_SEG=8): they were the default where 16-pixel segments leave SIMDs
  // of a frame's CU idle (W <= 2048, frames not sharing CUs: 64 x 1080p 7.83 ->
  // 6.32 ms in round 2), but the round-3/4 row kernel with 16-pixel segments is
  // as fast or faster at every width measured (round 4, profiles/r04v, r04y:
  // 64 x 1080p reconstruct 6.58 vs 6.88 ms, W = 1280 / 1024 / 640: 6.68 / 5.77
  // / 6.22 vs 6.91 / 6.00 / 6.30 ms)
  const uint32_t rows8_thr = ((w + 7) / 8 + 63) / 64 * 64;
  const size_t rows8_lds = rows_lds_bytes(rows8_thr, w, true);
  const bool rows8 = o.seg.set && o.seg.val == 8 && use_rows && rows_in_lds && rows8_thr <= ROWS_THREADS &&
                     lds_fits(rows8_lds);
  // wide frames, few of them: strips of <= 256 segments on separate CUs
  // (dec_rows_split; its blocks wait on each other, so they should all be
  // resident: at most one per CU for half the CUs, frames in chunks of that
  // many strips).  When they are not (other kernels hold the CUs), a strip's
  // wait times out and the frame goes to the fallback launch (dec_rows_wide,
  // or dec_reconstruct above 16384 columns) -- slower, never wrong.
  // NICE_DEC_SPLIT=k forces k strips (tests), =0 disables
  const uint32_t split_cap = (uint32_t)(s.cus / 2 > 1 ? s.cus / 2 : 1);
  uint32_t strips = (nseg16 + SPLIT_THREADS - 1) / SPLIT_THREADS;
  if (o.split.set) strips = (uint32_t)o.split.val;
  // <= 16384 columns: only when the whole batch fits at once (else one block
  // per frame is the better use of the CUs); wider: always, in frame chunks
  bool split = !single_wave && w >= 64 && strips >= 2 && strips <= split_cap &&
               (!use_rows || (uint64_t)n_frames * strips <= split_cap);
  // rows of up to 8192 pixels (8 waves) take the dataflow kernel on one CU
  // rather than strips on several (round 6: the strips' cross-CU hand-offs
  // cost more than the second CU gains); NICE_DEC_SPLIT forces the strips
  if (split && !o.split.set && use_rows && w <= FLOW_MAX_W && !o.seg.on() && !(o.flow.set && o.flow.val <= 0))
    split = false;
  const uint32_t sps = split ? (nseg16 + strips - 1) / strips : 0;   // segments per strip
  // every strip >= 2 segments (>= 3 pixels: its first and last three) and <= 256 lanes
  if (split && (sps > SPLIT_THREADS || nseg16 <= (strips - 1) * sps + 1)) split = false;
  // W <= 8192: the dataflow row kernel (no block barriers; dec_rows_flow).
  // At most one frame per CU: two row groups in flight and an 8-row ring (one
  // block per CU); larger batches: one group and a 4-row ring, so two frames
  // share each CU.  NICE_DEC_FLOW=0 takes dec_rows, =k forces k groups (A/B).
  uint32_t flow_k = 2, flow_ring = 8;
  bool flow = !split && use_rows && !rows8 && w <= FLOW_MAX_W;
  if (n_frames > cus) { flow_k = 1; flow_ring = 4; }
  if (o.flow.set) {
    const int v = (int)o.flow.val;
    if (v <= 0) flow = false;
    else flow_k = (uint32_t)v;
  }
  if (flow_k * rows_wpr > FLOW_THREADS / 64) flow_k = FLOW_THREADS / 64 / rows_wpr;
  if (flow_k > 4 || flow_k < 1) flow = false;   // (stamps of 8 rows)
  if (flow_k > 1) flow_ring = 8;
  if (!lds_fits(flow_lds_bytes(flow_ring, w)) && flow_k == 1) flow_ring = 4;   // wide rows: a 4-row ring (one row group)
  if (!lds_fits(flow_lds_bytes(flow_ring, w))) flow = false;

  const DecLaunch reconstruct{DEC_R_RECONSTRUCT, 64, g.lds};
  const DecLaunch rows_wide{DEC_R_ROWS_WIDE, rows_thr, rows_lds_bytes(rows_thr, w, false)};
  const DecLaunch rows{DEC_R_ROWS, rows_thr, rows_lds};
  p.fallback = DecLaunch{DEC_R_NONE, 0, 0};
  if (split) {
    p.strips = strips;
    p.split_frames = n_frames < split_cap / strips ? n_frames : split_cap / strips;
    p.hand = (size_t)n_frames * s.h * strips * SPLIT_GRAN * 8;
    // above 80 KB so a CU holds one strip
    const size_t lds = split_lds_bytes(sps * ROWS_SEG);
    p.rows = DecLaunch{DEC_R_SPLIT, SPLIT_THREADS, lds > 82 * 1024 ? lds : 82 * 1024};
    // frames whose strips timed out waiting for a non-resident neighbour
    p.fallback = use_rows ? rows_wide : reconstruct;
  } else if (flow) {
    p.flow_k = flow_k;
    p.flow_ring = flow_ring;
    p.rows = DecLaunch{DEC_R_FLOW, 64 * flow_k * rows_wpr, flow_lds_bytes(flow_ring, w)};
    // frames whose waits timed out (the workgroup was preempted or time-sliced
    // past the bound) go to the barrier kernel
    p.fallback = rows_in_lds ? rows : rows_wide;
  } else if (rows8) {
    p.rows = DecLaunch{DEC_R_ROWS8, rows8_thr, rows8_lds};
  } else if (use_rows) {
    p.rows = rows_in_lds ? rows : rows_wide;
  } else {
    p.rows = reconstruct;
  }
  // per-frame redo flags: the split kernel's, and the dataflow kernel's (a
  // wait that timed out sends the frame to the barrier kernel)
  p.abort_flags = split || flow;
  // the row ring in global memory: dec_rows_wide (also the split path's
  // fallback) or dec_reconstruct without room in LDS
  const size_t ring_rows = use_rows ? (size_t)n_frames * ROWS_RING * rows_ring_stride(w) * 4
                                    : (g.in_lds ? 0 : (size_t)n_frames * g.R * w * 4);
  p.rowbuf = split ? ring_rows : (use_rows && rows_in_lds) ? 0 : ring_rows;
  // rows so wide (W >= 39345) that dec_reconstruct's record row alone (4 bytes
  // per pixel) leaves no room in LDS, as the row kernel or as the strips'
  // fallback: no kernel takes the frame
  if (!lds_fits(p.rows.lds) || !lds_fits(p.fallback.lds)) p.rows = p.fallback = DecLaunch{DEC_R_NONE, 0, 0};
  return p;
}

}  // namespace nice
