// nice_slot_plan.hpp -- what a tiled or set decode does with every selected
// tile, decided by pure functions of the host tables and the windows: tile
// grids and window selection, the slots of M windows by kind with the statuses
// of the refused ones, and the one host buffer their columns are uploaded in.
// No HIP, no globals: a plain C++ compiler reads it too (tools/slot_plan_check.cpp,
// tests/test_slot_plan.py).  nice_capi.hip uploads, decodes and merges what the
// plan says; a tiled image is the set K = 1, M = 1, first = {0, n}.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/nice.h"
#include "nice_enc_plan.hpp"

namespace nice {

// ---- grids and selection (nice_tile_grid, nice_tile_select, nice_set_grid, nice_set_select) ----
inline int tile_grid(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t* nx, uint32_t* ny) {
  if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 30)) return NICE_E_ARG;
  if (tile_w < 2 || tile_h < 2 || tile_w > 8192 || tile_h > 8192) return NICE_E_ARG;
  const uint64_t gx = ((uint64_t)w + tile_w - 1) / tile_w, gy = ((uint64_t)h + tile_h - 1) / tile_h;
  // the batch encoder's 32-bit work counter: tiles x their 1024-pixel encoder tiles
  if (gx * gy * enc_tiles(tile_w, tile_h) >= (1ull << 32)) return NICE_E_ARG;
  *nx = (uint32_t)gx;
  *ny = (uint32_t)gy;
  return NICE_OK;
}

// The tiles [tx0, tx1) x [ty0, ty1) that a window overlaps.
struct TileRange {
  uint32_t tx0, ty0, tx1, ty1;
  uint64_t count() const { return (uint64_t)(tx1 - tx0) * (ty1 - ty0); }
};
// (the window is not empty and x0 + rw, y0 + rh fit 32 bits: tile_select checks)
inline TileRange window_tiles(uint32_t tile_w, uint32_t tile_h, uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh) {
  return {x0 / tile_w, y0 / tile_h, (x0 + rw - 1) / tile_w + 1, (y0 + rh - 1) / tile_h + 1};
}

inline int tile_select(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t x0, uint32_t y0, uint32_t rw,
                       uint32_t rh, uint32_t* nx, uint32_t* ny, TileRange* r) {
  int rc = tile_grid(w, h, tile_w, tile_h, nx, ny);
  if (rc) return rc;
  if (rw == 0 || rh == 0 || (uint64_t)x0 + rw > w || (uint64_t)y0 + rh > h) return NICE_E_ARG;
  *r = window_tiles(tile_w, tile_h, x0, y0, rw, rh);
  return NICE_OK;
}

// first[i]: image i's first global tile, first[K] the tiles of the set; nx[i]
// (nx may be null): its tiles per row.
inline int set_grid(const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                    uint32_t* first, uint32_t* nx) {
  if (!h_w || !h_h || !first || K == 0) return NICE_E_ARG;
  uint64_t n = 0;
  for (uint32_t i = 0; i < K; ++i) {
    uint32_t gx, gy;
    int rc = tile_grid(h_w[i], h_h[i], tile_w, tile_h, &gx, &gy);
    if (rc) return rc;
    first[i] = (uint32_t)n;
    if (nx) nx[i] = gx;
    n += (uint64_t)gx * gy;
    // the batch encoder's 32-bit work counter, over all tiles of the set
    if (n * enc_tiles(tile_w, tile_h) >= (1ull << 32)) return NICE_E_ARG;
  }
  first[K] = (uint32_t)n;
  return NICE_OK;
}

// The grid of the set (first: K + 1 entries, nx: K) and slot_first[j], window
// j's first slot; slot_first[M] the slots of the call.
inline int set_select(const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                      const uint32_t* h_win, uint32_t M, std::vector<uint32_t>& first, std::vector<uint32_t>& nx,
                      uint32_t* slot_first) {
  if (!h_win || !slot_first || M == 0) return NICE_E_ARG;
  first.resize((size_t)K + 1);
  nx.resize(K);
  int rc = set_grid(h_w, h_h, K, tile_w, tile_h, first.data(), nx.data());
  if (rc) return rc;
  uint64_t s = 0;
  for (uint32_t j = 0; j < M; ++j) {
    const uint32_t* q = h_win + 5ull * j;
    if (q[0] >= K) return NICE_E_ARG;
    uint32_t gx, gy;
    TileRange r;
    if ((rc = tile_select(h_w[q[0]], h_h[q[0]], tile_w, tile_h, q[1], q[2], q[3], q[4], &gx, &gy, &r))) return rc;
    slot_first[j] = (uint32_t)s;
    s += r.count();
    if (s >= (1ull << 32)) return NICE_E_ARG;
  }
  slot_first[M] = (uint32_t)s;
  return NICE_OK;
}

// ---- the slots of M windows -------------------------------------------------
// The host tables of a packed tile batch (val: the alpha batch's constants) and
// the bytes of the batch.
struct SlotTables {
  const uint64_t *off, *len;
  const uint8_t *kind, *val;
  uint64_t bytes;
};
// M windows {image, x0, y0, rw, rh} (checked: set_select) over images with
// first[i] and nx[i] as set_grid gives them.  with_win: the plan carries the
// window of every slot (a tiled call has one window and does not).
struct SlotWindows {
  uint32_t tile_w, tile_h;
  const uint32_t *first, *nx, *win;
  uint32_t M;
  bool with_win;
};
// Every (window, tile) pair is a slot; windows in the order given, the tiles of
// a window in raster order.  A slot's position counts every slot before it.
// Coded slots are decoded as one batch; the colour plan lists the raw slots
// besides (s_src: the offset), the alpha plan every accepted slot (s_src: the
// constant, the offset, or the index among the coded slots).  A refused slot
// is in no list: its status in init says why, and nothing touches its pixels.
struct SlotPlan {
  std::vector<uint64_t> c_off, c_len;          // coded: the stream in the batch
  std::vector<uint32_t> c_idx, c_win, c_pos;   // tile index in its image (colour), window, position
  std::vector<uint64_t> s_src;
  std::vector<uint32_t> s_idx, s_win;
  std::vector<uint8_t> s_kind;                 // (alpha)
  std::vector<int32_t> init;                   // the status of every slot before the decode
  uint32_t by_kind[3] = {0, 0, 0};             // accepted slots by kind
};

// f(position, window, tile index in the image, global tile) for every slot in order
template <class F>
inline void for_each_slot(const SlotWindows& g, F&& f) {
  uint32_t p = 0;
  for (uint32_t j = 0; j < g.M; ++j) {
    const uint32_t* q = g.win + 5ull * j;
    const uint32_t nx = g.nx[q[0]];
    const TileRange r = window_tiles(g.tile_w, g.tile_h, q[1], q[2], q[3], q[4]);
    for (uint32_t ty = r.ty0; ty < r.ty1; ++ty)
      for (uint32_t tx = r.tx0; tx < r.tx1; ++tx, ++p) f(p, j, ty * nx + tx, g.first[q[0]] + ty * nx + tx);
  }
}

inline bool slot_range_bad(uint64_t off, uint64_t len, uint64_t bytes) {
  return (off & 15) || off > bytes || len > bytes - off;
}

// Colour: kind 0 coded, kind 1 raw (3 bytes per pixel), anything else refused.
inline void plan_colour_slots(const SlotTables& t, const SlotWindows& g, SlotPlan& s) {
  const uint64_t npx = (uint64_t)g.tile_w * g.tile_h;
  for_each_slot(g, [&](uint32_t p, uint32_t j, uint32_t ti, uint32_t gt) {
    s.init.push_back(NICE_OK);
    const uint64_t off = t.off[gt], len = t.len[gt];
    const uint8_t k = t.kind[gt];
    if (k == 0) {   // (its offset and length are checked on the device, as for any packed batch)
      s.c_off.push_back(off);
      s.c_len.push_back(len);
      s.c_idx.push_back(ti);
      if (g.with_win) s.c_win.push_back(j);
      s.c_pos.push_back(p);
    } else if (k != 1) {
      s.init[p] = NICE_E_FORMAT;
      return;
    } else if (slot_range_bad(off, len, t.bytes)) {
      s.init[p] = NICE_E_ARG;
      return;
    } else if (len != 3 * npx) {
      s.init[p] = NICE_E_FORMAT;
      return;
    } else {
      s.s_src.push_back(off);
      s.s_idx.push_back(ti);
      if (g.with_win) s.s_win.push_back(j);
    }
    ++s.by_kind[k];
  });
}

// Alpha: kind 0 coded, kind 1 a raw plane (1 byte per pixel), kind 2 a constant.
inline void plan_alpha_slots(const SlotTables& t, const SlotWindows& g, SlotPlan& s) {
  const uint64_t npx = (uint64_t)g.tile_w * g.tile_h;
  for_each_slot(g, [&](uint32_t p, uint32_t j, uint32_t ti, uint32_t gt) {
    s.init.push_back(NICE_OK);
    const uint64_t off = t.off[gt], len = t.len[gt];
    const uint8_t k = t.kind[gt];
    if (k > 2) {
      s.init[p] = NICE_E_FORMAT;
      return;
    } else if (slot_range_bad(off, len, t.bytes)) {
      s.init[p] = NICE_E_ARG;
      return;
    } else if (k == 2 ? len != 0 : k == 1 ? len != npx : len == 0) {   // (no stream is empty)
      s.init[p] = NICE_E_FORMAT;
      return;
    } else if (k == 2) {
      s.s_src.push_back(t.val[gt]);
    } else if (k == 1) {
      s.s_src.push_back(off);
    } else {
      s.s_src.push_back(s.c_off.size());
      s.c_off.push_back(off);
      s.c_len.push_back(len);
      s.c_pos.push_back(p);
    }
    s.s_idx.push_back(ti);
    if (g.with_win) s.s_win.push_back(j);
    s.s_kind.push_back(k);
    ++s.by_kind[k];
  });
}

// ---- where every position's pixels are (the resize merge, nice_sets_resize.hip) ----
// src[p] of a colour plan, for every slot position p: bits 62-63 the kind, bits
// 0-61 the value.  Dense: 4 bytes per pixel, the value-th coded slot of the
// batch decode (in c_pos order); raw: 3 bytes per pixel at that byte offset of
// the packed batch (s_src, in order); none: refused by the plan, nothing to read.
constexpr uint64_t SLOT_SRC_DENSE = 0ull << 62, SLOT_SRC_RAW = 1ull << 62, SLOT_SRC_NONE = 3ull << 62;
constexpr uint64_t SLOT_SRC_VALUE = (1ull << 62) - 1;
inline void slot_position_sources(const SlotPlan& s, std::vector<uint64_t>& src) {
  src.assign(s.init.size(), SLOT_SRC_NONE);
  for (size_t k = 0; k < s.c_pos.size(); ++k) src[s.c_pos[k]] = SLOT_SRC_DENSE | (uint64_t)k;
  size_t r = 0;
  for (size_t p = 0; p < src.size(); ++p)
    if (src[p] == SLOT_SRC_NONE && s.init[p] == NICE_OK) src[p] = SLOT_SRC_RAW | (s.s_src[r++] & SLOT_SRC_VALUE);
}

// ---- one host buffer for the upload -------------------------------------------
// `head` (the callers' window descriptors; head_bytes a multiple of 8), then
// the plan's u64 columns, its u32 columns, its u8 column; host.size() == c_st,
// a multiple of 16, where the device keeps the coded slots' decode statuses
// (4 bytes each, up to `bytes`).  An empty column takes no room.
struct SlotTable {
  std::vector<uint8_t> host;
  size_t c_off, c_len, s_src, c_idx, c_win, c_pos, s_idx, s_win, s_kind, c_st, bytes;
};

template <class T>
inline size_t slot_table_add(std::vector<uint8_t>& host, const std::vector<T>& col) {
  const size_t o = host.size();
  host.resize(o + col.size() * sizeof(T));
  if (!col.empty()) memcpy(&host[o], col.data(), col.size() * sizeof(T));
  return o;
}

inline void pack_slot_table(const SlotPlan& s, const void* head, size_t head_bytes, SlotTable& t) {
  t.host.assign((const uint8_t*)head, (const uint8_t*)head + head_bytes);
  t.c_off = slot_table_add(t.host, s.c_off);
  t.c_len = slot_table_add(t.host, s.c_len);
  t.s_src = slot_table_add(t.host, s.s_src);
  t.c_idx = slot_table_add(t.host, s.c_idx);
  t.c_win = slot_table_add(t.host, s.c_win);
  t.c_pos = slot_table_add(t.host, s.c_pos);
  t.s_idx = slot_table_add(t.host, s.s_idx);
  t.s_win = slot_table_add(t.host, s.s_win);
  t.s_kind = slot_table_add(t.host, s.s_kind);
  t.host.resize((t.host.size() + 15) / 16 * 16);
  t.c_st = t.host.size();
  t.bytes = t.c_st + 4 * s.c_off.size();
}

}  // namespace nice
