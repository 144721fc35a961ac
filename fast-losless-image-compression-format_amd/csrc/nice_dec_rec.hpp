// nice_dec_rec.hpp -- the decoder's per-pixel record: what the record writers
// (dec_emit, dec_place: nice_decode.hip) store and the row kernels
// (nice_rows.hip) read, and the frame status both sides set.  Device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nice_format.h"

namespace nice {

// first error of a frame wins
__device__ __forceinline__ void set_status(int32_t* st, int32_t code) {
  atomicCAS(reinterpret_cast<int*>(st), 0, code);
}

// Record (round 6): the additive constant c in the row kernels' spread form
// (R | G << 10 | B << 20: bits 0..7, 10..17, 20..27), bits 28..31 the source
// class: 0 = AVG, 1..3 = the pixel 1..3 back in raster order (a run pixel is
// class 1 with c = 0), 4..13 = a pixel in a row above, at (rows back, pixels
// back) = cls_rows / cls_px.  The record writers (dec_emit, dec_place) spread
// the constant, so the row kernels' pre-pass -- on the row chain -- only masks
// it (round 5 kept bytes and spread every pixel there: ~5 VALU per pixel).
constexpr uint32_t REC_RUN = 1u << 28;
constexpr uint32_t REC_K = 0xFFu | (0xFFu << 10) | (0xFFu << 20);   // the constant's bits
// Records written by a decode call carry its tag (1..15) in the gap bits 8..9
// (tag & 3) and 18..19 (tag >> 2); a slot without the current tag (stale, or
// cleared to 0) is a run pixel.  The record buffer is then cleared only when
// its tags wrap or its layout changes (nice_capi.hip), not prefilled with
// REC_RUN by every call.  The canonical record keeps the tag bits: readers take
// the class (rec_cls) and the constant (rec_c) only.
constexpr uint32_t REC_TAG_MASK = (3u << 8) | (3u << 18);
__device__ __forceinline__ uint32_t rec_tagbits(uint32_t tag) { return ((tag & 3u) << 8) | ((tag >> 2) << 18); }
__device__ __forceinline__ uint32_t rec_canon(uint32_t r, uint32_t tag) {
  return (r & REC_TAG_MASK) == rec_tagbits(tag) ? r : REC_RUN;
}
__device__ __forceinline__ uint32_t rec_cls(uint32_t r) { return r >> 28; }
__device__ __forceinline__ uint32_t rec_c(uint32_t r) { return r & REC_K; }
// R | G << 8 | B << 16 -> spread (the record writers)
__device__ __forceinline__ uint32_t rec_spread(uint32_t v) {
  return (v & 0xFFu) | ((v & 0xFF00u) << 2) | ((v & 0xFF0000u) << 4);
}
__host__ __device__ constexpr int cls_rows(int c) {
  return c < 4 ? 0 : c == 4 ? 1 : c == 5 ? 1 : c == 6 ? 2 : c == 7 ? 1 : c <= 10 ? 3 : c == 11 ? 1 : c <= 13 ? 3 : 0;
}
__host__ __device__ constexpr int cls_px(int c) {
  return c < 4 ? c : c == 4 ? 0 : c == 5 ? -1 : c == 6 ? 0 : c == 7 ? -3 : c == 8 ? -1 : c == 9 ? 0
       : c == 10 ? 1 : c == 11 ? 3 : c == 12 ? 3 : c == 13 ? -3 : 0;
}
// reference id (back refs 0..4, luma refs 5..15) -> class
__host__ __device__ constexpr int id_cls(int id) {
  return id == 0 ? 1 : id == 1 ? 4 : id == 2 ? 5 : id == 3 ? 2 : id == 4 ? 6
       : id == 5 ? 1 : id == 6 ? 4 : id == 7 ? 5 : id == 8 ? 7 : id == 9 ? 3 : id == 10 ? 8
       : id == 11 ? 9 : id == 12 ? 10 : id == 13 ? 11 : id == 14 ? 12 : 13;
}
__host__ __device__ constexpr bool cls_table_ok() {
  for (int id = 0; id < 16; ++id) {
    const int rows = id < 5 ? br_rows(id) : lr_rows(id - 5), px = id < 5 ? br_px(id) : lr_px(id - 5);
    if (cls_rows(id_cls(id)) != rows || cls_px(id_cls(id)) != px) return false;
  }
  return true;
}
static_assert(cls_table_ok(), "reference offsets (code.rs:141-145) map onto the record classes");
constexpr unsigned long long ID_CLS_PACK = [] {
  unsigned long long v = 0;
  for (int id = 0; id < 16; ++id) v |= (unsigned long long)id_cls(id) << (4 * id);
  return v;
}();
constexpr uint32_t CLS_ROWS_PACK = [] {
  uint32_t v = 0;
  for (int c = 0; c < 16; ++c) v |= (uint32_t)cls_rows(c) << (2 * c);
  return v;
}();
constexpr unsigned long long CLS_PX_PACK = [] {
  unsigned long long v = 0;
  for (int c = 0; c < 16; ++c) v |= (unsigned long long)(cls_px(c) + 3) << (3 * c);
  return v;
}();

}  // namespace nice
