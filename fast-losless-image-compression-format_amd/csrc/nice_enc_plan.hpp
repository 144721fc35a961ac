// nice_enc_plan.hpp -- what one encode call (a batch of frames, or one band of
// a sharded image) launches, decided by a pure function of the shape and the
// test options: no HIP, no globals (tools/enc_plan_check.cpp drives it on the
// CPU).  nice_capi.hip only allocates and launches what the plan says.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "nice_format.h"
#include "nice_geom.h"

namespace nice {

struct EncShape {
  uint32_t n_frames, w, h;
  uint8_t channels;
  int cus;                   // compute units of the device
  // pixel memory (frames: the base, and the stride when n_frames > 1; bands:
  // the virtual base) is 4-byte / 16-byte aligned
  bool aligned4, aligned16;
  // one band of a sharded image (n_frames == 1): tiles [tile_lo, tile_hi);
  // frames take every tile
  bool band;
  uint32_t tile_lo, tile_hi;
};
// The NICE_OPT_ENC_* test / A/B options (include/nice_test.h) as plain values.
struct EncOpts { bool no_ring, no_pair, no_slide; };

// the classify kernels (nice_test_last_classify reports these values)
enum ClsKind : int { CLS_K_WINDOW, CLS_K_TINY, CLS_K_RING, CLS_K_RING2, CLS_K_STRIP, CLS_K_PAIR, CLS_K_TWIN, CLS_K_SLIDE };

// One kernel launch: grid (x, y) and block size; x == 0: not launched.
struct EncLaunch {
  uint32_t x, y, threads;
  bool on() const { return x != 0; }
};
struct EncPlan {
  uint32_t tiles_per_frame, tile_lo, tile_hi;
  // classify: the kernel is (kind, rgb, flags_out, wmod4); tiles_per_block is
  // EncArgs::tiles_per_block (the strip kernel: rows per block)
  ClsKind kind;
  bool rgb;            // 3 bytes per pixel
  bool flags_out;      // the _m forms: coded flags out, run digits by enc_rundigits
  uint32_t wmod4;      // enc_classify_slide0..3
  EncLaunch classify;
  uint32_t tiles_per_block;
  EncLaunch rundigits;
  int il;              // enc_rundigits: the flags are in the slide kernel's ballot order
  uint32_t cmask_std;  // EncArgs::cmask_std: enc_pack reads the coded flags
  // tile scans: `groups` blocks of ENC_GROUP_TILES tiles per frame
  uint32_t groups;
  EncLaunch group_reduce, tailruns, tilescan;
  EncLaunch tables, header, packtab;
  EncLaunch long_path;   // enc_tilebits and both enc_pack_long phases
  EncLaunch pack;
  uint32_t pack_slots;   // EncArgs::pack_slots: frames enc_pack works at once
  EncLaunch pack_over, edges, tail;
};

constexpr uint32_t enc_tiles(uint32_t w, uint32_t h) {
  return (uint32_t)(((uint64_t)w * h + ENC_TILE - 1) / ENC_TILE);
}

// The classify kernel for a shape (every kernel writes the same records,
// histogram and tile edges): the LDS ring (each pixel loaded once) wherever
// the rows fit it -- RGBA rows that also leave room for a second tile take the
// pair kernel, and frames (not bands) in 16-byte aligned memory the per-lane
// sliding-window kernel -- the strip kernel for wider RGBA rows of whole tiles,
// the 32K ring, per-tile row windows for every other wide shape, and the
// round-1 window kernel for pixel memory that is not 4-byte aligned, which the
// ring, strip and tile-window loads need.
inline ClsKind pick_classify(const EncShape& s, const EncOpts& o) {
  const uint32_t w = s.w;
  if (w < 3) return CLS_K_TINY;
  if (!s.aligned4 || o.no_ring) return CLS_K_WINDOW;
  const bool pair = s.channels == 4 && w <= CLS_PAIR_MAX_W && !o.no_pair;   // no_pair: one tile per iteration (A/B)
  if (pair && !s.band && s.aligned16 && !o.no_slide) return CLS_K_SLIDE;
  if (pair) return CLS_K_PAIR;
  if (w <= CLS_RING_MAX_W) return CLS_K_RING;
  if (s.channels == 4 && w % ENC_TILE == 0) return CLS_K_STRIP;
  if (w <= CLS_RING2_MAX_W) return CLS_K_RING2;
  return CLS_K_TWIN;
}

inline EncPlan plan_encode(const EncShape& s, const EncOpts& o) {
  EncPlan p{};
  const uint32_t n_frames = s.n_frames, w = s.w;
  const uint64_t cus = (uint64_t)(s.cus > 1 ? s.cus : 1);
  const uint32_t T = p.tiles_per_frame = enc_tiles(w, s.h);
  p.tile_lo = s.band ? s.tile_lo : 0;
  p.tile_hi = s.band ? s.tile_hi : T;
  const uint32_t nt = p.tile_hi - p.tile_lo;    // tiles of each frame (of the band)
  const uint64_t work = (uint64_t)n_frames * nt;
  auto min64 = [](uint64_t a, uint64_t b) { return a < b ? a : b; };
  auto launch = [](uint64_t x, uint32_t y, int threads) { return EncLaunch{(uint32_t)x, y, (uint32_t)threads}; };

  p.groups = nt ? (nt + ENC_GROUP_TILES - 1) / ENC_GROUP_TILES : 1;
  {   // frames packed at once: <= 64, dividing the frames about evenly
    const uint32_t per = (n_frames + 63) / 64;
    p.pack_slots = per ? (n_frames + per - 1) / per : 0;
  }
  if (n_frames == 0) return p;
  p.tables = launch((uint64_t)n_frames * N_STREAMS, 1, ENC_WAVE_THREADS);
  p.header = launch(n_frames, 1, ENC_WAVE_THREADS);
  p.kind = pick_classify(s, o);
  p.rgb = s.channels == 3;
  p.wmod4 = w & 3u;
  if (work == 0) return p;   // empty frames: tables and header only

  // ---- classify: contiguous tile chunks per block (keeps rows-above reuse in
  // L2 and flushes each block's LDS histogram once per frame)
  const ClsKind k = p.kind;
  const bool staged = k != CLS_K_WINDOW && k != CLS_K_TINY;
  p.flags_out = staged && !s.band;   // bands: the kernels count their run digits themselves
  if (k == CLS_K_STRIP) {
    // rows per block: about three blocks per CU over all frames and strips,
    // >= 16 rows so the 3-row prefill stays small.  Bands walk their own rows
    // (tiles outside the band are staged, not classified).
    const uint32_t tpr = w / ENC_TILE;   // >= 1: W % ENC_TILE == 0, W > CLS_RING_MAX_W
    const uint32_t rows = s.band ? (p.tile_hi + tpr - 1) / tpr - p.tile_lo / tpr : s.h;
    const uint64_t strips = (w + STRIP_W - 1) / STRIP_W, want = 3 * cus;
    uint64_t r = (rows * strips * n_frames + want - 1) / want;
    if (r < 16) r = 16;
    if (r > rows) r = rows ? rows : 1;
    p.tiles_per_block = (uint32_t)r;
    p.classify = launch(n_frames * strips * ((rows + r - 1) / r), 1, CLS_THREADS);
  } else if (k == CLS_K_TWIN) {
    const uint64_t per = (work + 2 * cus - 1) / (2 * cus);
    p.tiles_per_block = (uint32_t)per;
    p.classify = launch((work + per - 1) / per, 1, CLS_THREADS);
  } else {
    // ring kernels: 2 blocks per CU (ring2: 1, its ring is twice the LDS),
    // >= 16 tiles per block (the 3-row prefill amortised), <= 16384 (their
    // 16-bit per-thread prefix counters); window kernels: 2048 blocks
    const uint64_t blocks = !staged ? 2048 : k == CLS_K_RING2 ? cus : 2 * cus;
    uint64_t per = (work + blocks - 1) / blocks;
    if (staged && per < 16) per = 16;
    if (staged && per > 16384) per = 16384;
    p.tiles_per_block = (uint32_t)per;
    p.classify = launch((work + per - 1) / per, 1, staged ? CLS_THREADS : ENC_THREADS);
  }
  if (p.flags_out) {   // in-tile run digits, from the coded flags (>= 2048 blocks in all for few, large frames)
    const uint32_t most = 2048u / n_frames > 64u ? 2048u / n_frames : 64u;
    p.rundigits = launch(min64((T + 7) / 8, most), n_frames, RUNDIGITS_THREADS);
    p.il = k == CLS_K_SLIDE ? 1 : 0;
    p.cmask_std = 1;
  }

  // ---- runs crossing tile ends, tables, pack
  if (p.groups > 1) p.group_reduce = launch(p.groups, n_frames, GROUP_THREADS);
  p.tailruns = launch(p.groups, n_frames, TR_THREADS);
  p.tilescan = launch(p.groups, n_frames, SCAN_THREADS);
  p.packtab = launch(n_frames, 1, PACKTAB_THREADS);
  p.long_path = launch(min64(work, ENC_LONG_BLOCKS), 1, ENC_THREADS);
  p.pack = launch(min64(work, cus * PACK_BLOCKS_PER_CU), 1, PK_THREADS);
  p.pack_over = launch(PACK_OVER_BLOCKS, 1, PK_THREADS);
  // enc_edges: a thread per enc_pack group (PACK_SUB tiles), blocks striding.
  // Frames size the grid from the tiles, about four times the blocks the
  // groups need (the extra ones find nothing to do); bands from the groups.
  // Kept as it was: the launches of a refactored host must not move.
  const uint32_t edge_items = s.band ? (nt + PACK_SUB - 1) / PACK_SUB : T;
  p.edges = launch(min64((edge_items + 255) / 256, 64), (uint32_t)min64(n_frames, 4096), EDGES_THREADS);
  p.tail = launch((n_frames + 63) / 64, 1, ENC_WAVE_THREADS);
  return p;
}

}  // namespace nice
