// nice_geom.h -- the one definition of every constant and LDS layout that both
// a kernel and the host's launch planning (nice_enc_plan.hpp, nice_dec_plan.hpp,
// nice_capi.hip) depend on.  No HIP: a plain C++ compiler reads it too
// (tests/test_enc_plan.py, tests/test_classify_routes.py, tests/test_dec_plan.py,
// tests/test_dec_route.py; through nice_slot_plan.hpp, tests/test_slot_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

// NICE_HDI: host and device under hipcc (always inlined in a kernel), plain inline elsewhere
#if defined(__HIPCC__) || defined(__CUDACC__)
#define NICE_HD __host__ __device__
#define NICE_HDI __host__ __device__ __forceinline__
#else
#define NICE_HD
#define NICE_HDI inline
#endif

namespace nice {

// LDS of one workgroup on gfx950 (static + dynamic); dynamic LDS above
// LDS_OPT_IN needs hipFuncAttributeMaxDynamicSharedMemorySize
constexpr uint32_t LDS_BUDGET = 160 * 1024, LDS_OPT_IN = 64 * 1024;
// a launch's dynamic LDS fits beside up to 1 KB of static LDS (class tables, flags)
NICE_HD constexpr bool lds_fits(size_t dynamic_bytes) { return dynamic_bytes + 1024 <= LDS_BUDGET; }

// ---- encoder classify kernels (nice_classify.hip) ---------------------------
constexpr int ENC_TILE = 1024;     // pixels per encoder tile (raster-contiguous)
constexpr int ENC_THREADS = 256;   // enc_classify / _tiny (window kernels), enc_tilebits, enc_pack_long
constexpr int CLS_THREADS = 512;   // block size of every ring / pair / slide / strip / twin classify kernel
constexpr int STRIP_W = 2048;      // enc_classify_strip: columns per strip
constexpr int CLS_RING = 16384;    // ring words (64 KB); enc_classify_ring2: twice that
// Widest rows a ring takes: it holds 3W + 3 pixels of references plus `tiles`
// tiles (the one being classified and the next one being staged; the pair
// kernel works two at a time): 3W + 3 + tiles * ENC_TILE <= ring
constexpr uint32_t cls_ring_max_w(int ring, int tiles) { return (uint32_t)((ring - tiles * ENC_TILE - 3) / 3); }
constexpr uint32_t CLS_RING_MAX_W = cls_ring_max_w(CLS_RING, 2);        // enc_classify_ring / ring3
constexpr uint32_t CLS_RING2_MAX_W = cls_ring_max_w(2 * CLS_RING, 2);   // enc_classify_ring2 / ring2_3
constexpr uint32_t CLS_PAIR_MAX_W = cls_ring_max_w(CLS_RING, 4);        // enc_classify_pair, enc_classify_slide
static_assert(CLS_RING_MAX_W == 4777, "16K ring");
static_assert(CLS_RING2_MAX_W == 10239, "32K ring");
static_assert(CLS_PAIR_MAX_W == 4095, "16K ring, two tiles per iteration");
constexpr int RUNDIGITS_THREADS = 256;   // enc_rundigits

// ---- encoder scans, tables (nice_encode.hip) and pack (nice_pack.hip) -------
// the per-frame tile scans (enc_tailruns, enc_tilescan) run as blocks of
// ENC_GROUP_TILES tiles; enc_group_reduce gives each group's aggregate
constexpr uint32_t ENC_GROUP_TILES = 8192;
constexpr int GROUP_THREADS = 256;    // enc_group_reduce
constexpr int TR_THREADS = 1024;      // enc_tailruns
constexpr int SCAN_THREADS = 1024;    // enc_tilescan
constexpr int ENC_WAVE_THREADS = 64;  // one wave: enc_tables, enc_header, enc_tail, enc_band_check, enc_band_fix
constexpr int PACKTAB_THREADS = 256;  // enc_packtab
constexpr int BAND_THREADS = 256;     // enc_band_edges, enc_band_sum, enc_band_merge
#ifndef NICE_PACK_BPC
#define NICE_PACK_BPC 4
#endif
#ifndef NICE_PACK_CAP_BPP
#define NICE_PACK_CAP_BPP 32     // enc_pack's LDS group buffer: bits per pixel
#endif
constexpr int PK_THREADS = 256;                          // enc_pack, enc_pack_over
constexpr uint32_t PACK_BLOCKS_PER_CU = NICE_PACK_BPC;   // enc_pack: a persistent grid, ~35 KB LDS per block
constexpr int PACK_SUB = 4;                              // tiles per enc_pack work item (group)
constexpr uint32_t PACK_OVER_BLOCKS = 64;   // enc_pack_over's grid (blocks loop over the listed groups)
constexpr int EDGES_THREADS = 256;          // enc_edges
constexpr uint32_t ENC_LONG_BLOCKS = 2048;  // enc_tilebits / enc_pack_long: at most (blocks take tile ranges)

// ---- decoder parse (nice_decode.hip) ----------------------------------------
// sync checkpoint spacing inside a slice (DecArgs::ck_bits, chosen per call:
// at most one emit sub-slice; 128: +30 % dec_sync -- scattered stores)
constexpr uint32_t DEC_CK_BITS = 1024;      // slices of 8K bits and more (the bench's 512 x 4K)
constexpr uint32_t DEC_CK_BITS_SMALL = 512;  // shorter slices (small batches)
constexpr uint32_t DEC_MIN_CHUNK_BITS = 1024;   // speculative-parse slice: a power of two
constexpr uint32_t DEC_MAX_CHUNK_BITS = 16384;  // chosen per call (plan_decode)
constexpr uint32_t DEC_EMIT_BITS = 1024;        // record-emission sub-slice (<= the slice)
constexpr int DEC_MAX_SEGS = 64;            // dec_reconstruct: one lane per row segment
constexpr uint32_t SETTLE_THREADS = 512;    // dec_sync_settle's block (it partitions a frame's slices by it)

// ---- decoder row kernels ----------------------------------------------------
constexpr int ROWS_SEG = 16;        // pixels per lane
constexpr uint32_t ROWS_RING = 4;   // rows y-4 .. y-1 while row y is built
constexpr uint32_t ROWS_RB = 4;     // left halo words before pixel 0
constexpr uint32_t ROWS_THREADS = 512, ROWS_WIDE_THREADS = 1024;   // launch bounds: dec_rows / dec_rows8, dec_rows_wide
// Ring row: W pixels padded one word per 16 (pixel x at x + (x >> 4)), plus 16
// spare words that take a partial last segment's padding pixels (stored
// unmasked), and halos so that no reference needs wrap logic: words -4..-2 hold
// the previous row's last three pixels (x = -3..-1), words g(W..W+2) the next
// row's first three (written when that row is emitted; the spare words of the
// previous use are overwritten by then).
NICE_HD constexpr uint32_t rows_ring_stride(uint32_t W) { return W + (W >> 4) + 24; }
// dec_rows_body's dynamic LDS, in words from its base: per lane {lo, len} x 3
// tails and one flag, the row's first three pixels, two round flags, the error
// word; then (dec_rows, dec_rows8) the ring.  dec_rows_wide keeps the ring in
// global memory.
struct RowsLds { uint32_t tails, flags, head3, pend, err, ring; };
NICE_HD constexpr RowsLds rows_lds(uint32_t nthr) {
  return {0, nthr * 6, nthr * 7, nthr * 7 + 4, nthr * 7 + 6, nthr * 7 + 8};
}
NICE_HD constexpr size_t rows_lds_bytes(uint32_t nthr, uint32_t W, bool lds_ring) {
  return ((size_t)rows_lds(nthr).ring + (lds_ring ? (size_t)ROWS_RING * rows_ring_stride(W) : 0)) * 4;
}

// dec_rows_flow: its control block, then a ring of 4 or 8 rows
constexpr uint32_t FLOW_THREADS = 512;
constexpr uint32_t FLOW_SLOTS = 8;   // stamp slots
constexpr uint32_t FLOW_MAXW = 8;    // waves per row: W <= 8192 (round 6; 4 before)
constexpr uint32_t FLOW_MAX_W = FLOW_MAXW * 64 * ROWS_SEG;
struct alignas(8) FlowPair { uint32_t x, y; };   // a uint2 to the kernel
struct FlowCtl {
  uint32_t fin[FLOW_SLOTS][FLOW_MAXW];
  uint32_t tst[FLOW_SLOTS][FLOW_MAXW];
  uint32_t tail[FLOW_SLOTS][FLOW_MAXW][4];
  uint32_t hst[FLOW_SLOTS];
  uint32_t head[FLOW_SLOTS][4];
  FlowPair rtab[FLOW_THREADS / 64][16];   // per wave: the class table of its current row
  uint32_t zero[4];                       // the "reference" word of records that have none
  int err;
  uint32_t abort;
  uint32_t pad[2];
};
static_assert(sizeof(FlowCtl) % 16 == 0, "ring after the control block, 16-byte aligned");
NICE_HD constexpr size_t flow_lds_bytes(uint32_t ring_rows, uint32_t W) {
  return sizeof(FlowCtl) + ((size_t)ring_rows * rows_ring_stride(W) + ROWS_RB) * 4;
}

// dec_rows_split: per lane tails and a flag as above, 4 words, then a 4-row
// ring of the strip's sw columns plus three halo columns on each side
constexpr uint32_t SPLIT_THREADS = 256;   // lanes (16-pixel segments) per strip
constexpr uint32_t SPLIT_GRAN = 8;        // granules per unit: first3 at 0..2, last3 at 4..6
NICE_HD constexpr uint32_t split_ring_stride(uint32_t sw) { return (sw + 6) + ((sw + 6) >> 4) + 17; }
constexpr uint32_t SPLIT_FLAGS = SPLIT_THREADS * 6, SPLIT_RING = SPLIT_THREADS * 7 + 4;   // word offsets
NICE_HD constexpr size_t split_lds_bytes(uint32_t sw) {
  return ((size_t)SPLIT_RING + (size_t)ROWS_RING * split_ring_stride(sw)) * 4;
}

}  // namespace nice
