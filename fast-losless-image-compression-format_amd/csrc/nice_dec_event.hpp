// nice_dec_event.hpp -- the decoder's integer arithmetic between the parse and
// the row kernels: the per-pixel record's layout and class tables, the event
// word dec_sync keeps per parsed pixel (ev_pack), the record dec_emit builds
// from a pixel's symbols (make_record: the yardstick) and the record dec_place
// builds from an event word (place_record).  No HIP header: a plain C++
// compiler reads it too, so the CPU check of this arithmetic
// (tools/dec_event_check.cpp, tests/test_dec_event_arith.py) runs the functions
// the kernels of nice_decode.hip run.
#pragma once
#include <stdint.h>

#include "nice_format.h"

namespace nice {

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
NICE_HDI uint32_t rec_tagbits(uint32_t tag) { return ((tag & 3u) << 8) | ((tag >> 2) << 18); }
NICE_HDI uint32_t rec_canon(uint32_t r, uint32_t tag) {
  return (r & REC_TAG_MASK) == rec_tagbits(tag) ? r : REC_RUN;
}
NICE_HDI uint32_t rec_cls(uint32_t r) { return r >> 28; }
NICE_HDI uint32_t rec_c(uint32_t r) { return r & REC_K; }
// R | G << 8 | B << 16 -> spread (the record writers)
NICE_HDI uint32_t rec_spread(uint32_t v) {
  return (v & 0xFFu) | ((v & 0xFF00u) << 2) | ((v & 0xFF0000u) << 4);
}
NICE_HD constexpr int cls_rows(int c) {
  return c < 4 ? 0 : c == 4 ? 1 : c == 5 ? 1 : c == 6 ? 2 : c == 7 ? 1 : c <= 10 ? 3 : c == 11 ? 1 : c <= 13 ? 3 : 0;
}
NICE_HD constexpr int cls_px(int c) {
  return c < 4 ? c : c == 4 ? 0 : c == 5 ? -1 : c == 6 ? 0 : c == 7 ? -3 : c == 8 ? -1 : c == 9 ? 0
       : c == 10 ? 1 : c == 11 ? 3 : c == 12 ? 3 : c == 13 ? -3 : 0;
}
// reference id (back refs 0..4, luma refs 5..15) -> class
NICE_HD constexpr int id_cls(int id) {
  return id == 0 ? 1 : id == 1 ? 4 : id == 2 ? 5 : id == 3 ? 2 : id == 4 ? 6
       : id == 5 ? 1 : id == 6 ? 4 : id == 7 ? 5 : id == 8 ? 7 : id == 9 ? 3 : id == 10 ? 8
       : id == 11 ? 9 : id == 12 ? 10 : id == 13 ? 11 : id == 14 ? 12 : 13;
}
NICE_HD constexpr bool cls_table_ok() {
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

// ---------------------------------------------------------------------------
// dec_emit's record, from a pixel's symbols (code.rs:579-644).
// ---------------------------------------------------------------------------
// A coded pixel's record before its tag carries, in two of the gap bits that
// later take the tag, EV_L2 (LUMA2: needs the row above) and EV_BAD
// (make_event_rec, rec_bad_at).
constexpr uint32_t EV_BAD = 1u << 9, EV_L2 = 1u << 8;

// Record of a completed coded pixel (branch-free), as an event word: the
// record in its spread layout (REC_K: the constant in bits 0-7, 10-17 and
// 20-27; the class in bits 28-31) with, in two of the gap bits that later
// take the call's tag (REC_TAG_MASK: bits 8-9 and 18-19), EV_L2 (bit 8, LUMA2:
// needs the row above) and EV_BAD (bit 9: an index the reference rejects
// wherever the pixel is, or an offset that wraps for W < 3).  The
// position-dependent checks are rec_bad_at's.
NICE_HDI uint32_t make_event_rec(uint64_t W, uint32_t mode, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3) {
  const bool isbr = mode == P_BACK_REF, islu = mode == P_LUMA;
  const bool issd = mode == P_SMALL_DIFF, isl2 = mode == P_LUMA2;
  const uint32_t idr = isbr ? s0 : 5u + s0;
  const uint32_t id = idr < 15u ? idr : 15u;
  const uint32_t cls = (uint32_t)(ID_CLS_PACK >> (4 * id)) & 15u;
  const uint64_t rows = (CLS_ROWS_PACK >> (2 * cls)) & 3u;
  const int64_t off = (int64_t)(rows * W) + (int64_t)((CLS_PX_PACK >> (3 * cls)) & 7u) - 3;
  const bool bad0 = (isbr && s0 >= 5u) || (islu && s0 >= 11u) || off < 0;
  const uint32_t gl = (s1 - 32u) & 255u;
  const uint32_t c_lu = ((s2 - 16u + gl) & 255u) | (gl << 10) | (((s3 - 16u + gl) & 255u) << 20);
  const uint32_t rd = s0 % 7u, t1 = s0 / 7u;
  const uint32_t c_sd = ((rd - 3u) & 255u) | ((((t1 % 7u) - 3u) & 255u) << 10) | ((((t1 / 7u) - 3u) & 255u) << 20);
  const uint32_t g2 = (s0 - 32u) & 255u;
  const uint32_t c_l2 = ((s1 - 16u + g2) & 255u) | (g2 << 10) | (((s2 - 16u + g2) & 255u) << 20);
  const uint32_t c_rgb = (s0 & 255u) | ((s1 & 255u) << 10) | ((s2 & 255u) << 20);
  const uint32_t r = (isbr || islu) ? ((cls << 28) | (islu ? c_lu : 0u)) : issd ? c_sd : isl2 ? c_l2 : c_rgb;
  return r | (isl2 ? EV_L2 : 0u) | ((isbr || islu) && bad0 ? EV_BAD : 0u);
}
// The reference panics on this pixel at position q: a reference before the
// image start (code.rs:141-145 offsets) or LUMA2 on the first row (code.rs:583).
NICE_HDI bool rec_bad_at(uint32_t ev, uint64_t q, uint64_t W) {
  const uint32_t cls = rec_cls(ev);
  const uint64_t rows = (CLS_ROWS_PACK >> (2 * cls)) & 3u;
  const uint64_t off = rows * W + ((CLS_PX_PACK >> (3 * cls)) & 7u) - 3u;   // >= 0 unless EV_BAD
  return (ev & EV_BAD) || ((ev & EV_L2) ? q < W : (cls != 0u && q < off));
}
NICE_HDI uint32_t make_record(uint64_t W, uint64_t q, uint32_t mode, uint32_t s0, uint32_t s1, uint32_t s2,
                              uint32_t s3, bool& bad) {
  const uint32_t ev = make_event_rec(W, mode, s0, s1, s2, s3);
  bad = rec_bad_at(ev, q, W);
  return ev & ~(EV_L2 | EV_BAD);
}

// ---------------------------------------------------------------------------
// The event word dec_sync keeps per parsed pixel, and dec_place's record from it.
// ---------------------------------------------------------------------------
// A run digit's event is EV_RUN | pixels (saturated).  A coded pixel's has its
// prefix in bits 28-30 and its payload symbols where the record wants them, so
// dec_place masks and adds instead of extracting and re-packing fields:
//   RGB         R, G, B in the record's fields f0 / f1 / f2 (bits 0-7, 10-17,
//               20-27): the record constant as it stands
//   LUMA2       the base (G) symbol in f1, the R and B symbols in f0 and f2
//   LUMA        the same three roles, and the reference (0..10) in bits 16-19:
//               the base symbol is < 64, so f1's top two bits and the gap
//               above it are free
//   BACK_REF    the reference id in bits 16-19, where LUMA's reference is
//   SMALL_DIFF  the index (< 343) in bits 0-8
// (The reference split over the four gap bits 8-9 / 18-19 was the first plan;
// one 4-bit field costs dec_sync one shift instead of three operations and
// dec_place one extraction instead of three, and both layouts need the same
// one mask before the luma sum.)
constexpr uint32_t EV_RUN = 1u << 31;
constexpr uint32_t EV_PFX_SHIFT = 28, EV_ID_SHIFT = 16;
// where payload symbol i of a prefix goes (symbols a mode does not have are 0)
NICE_HD constexpr uint32_t ev_shift(uint32_t pfx, uint32_t i) {
  return pfx == (uint32_t)P_BACK_REF ? (i == 0 ? EV_ID_SHIFT : 0u)
       : pfx == (uint32_t)P_RGB ? (i == 0 ? 0u : i == 1 ? 10u : i == 2 ? 20u : 0u)
       : pfx == (uint32_t)P_LUMA ? (i == 0 ? EV_ID_SHIFT : i == 1 ? 10u : i == 2 ? 0u : 20u)
       : pfx == (uint32_t)P_LUMA2 ? (i == 0 ? 10u : i == 1 ? 0u : i == 2 ? 20u : 0u)
       : 0u;
}
NICE_HDI uint32_t ev_pack(uint32_t pfx, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3) {
  return (pfx << EV_PFX_SHIFT) | (s0 << ev_shift(pfx, 0)) | (s1 << ev_shift(pfx, 1)) | (s2 << ev_shift(pfx, 2)) |
         (s3 << ev_shift(pfx, 3));
}

// dec_place's table, one entry per (reference id field, prefix): entry
// (id << 3) | prefix (the five prefixes of a wave's events are then
// neighbours in LDS, not 16 entries -- every bank -- apart).  An entry says how
// the event word becomes a record without a compare or a select on the prefix:
//   record = cls | (luma sum & ml) | (event & mr) | sdl[(event & msd) | (343 & ~msd)]
// cls: the reference's class << 28 (BACK_REF, LUMA), else 0;  ml: REC_K for the
// two luma modes;  mr: REC_K for RGB;  msd: 511 for SMALL_DIFF (else the gather
// reads entry 343 of the SMALL_DIFF table, which is 0).  A reference id the
// reference rejects wherever the pixel is (BACK_REF id >= 5, LUMA reference
// >= 11, an offset that wraps for W < 3) has mr == EV_BAD -- bit 9 of a
// BACK_REF or LUMA event is 0, so the record is unchanged -- and the offset
// 0xFFFFFFFF.  off3[entry]: the pixels the event needs before it, plus 3: the
// reference's offset rows * W + px, W for LUMA2 (the row above), else 0;
// `q + 3 < off3` is every position check at once.
struct alignas(16) PlaceEnt {
  uint32_t cls, ml, mr, msd;
};
constexpr uint32_t PLACE_ENTRIES = 128;
NICE_HDI PlaceEnt place_entry(uint32_t entry, uint32_t W, uint32_t& off3) {
  const uint32_t pfx = entry & 7u, idf = entry >> 3;
  const bool isbr = pfx == (uint32_t)P_BACK_REF, islu = pfx == (uint32_t)P_LUMA;
  const bool isl2 = pfx == (uint32_t)P_LUMA2;
  const uint32_t idr = isbr ? idf : 5u + idf;
  const uint32_t id = idr < 15u ? idr : 15u;   // as make_event_rec
  const uint32_t cls = (uint32_t)(ID_CLS_PACK >> (4u * id)) & 15u;
  const uint32_t o3 = (uint32_t)((CLS_ROWS_PACK >> (2u * cls)) & 3u) * W + (uint32_t)((CLS_PX_PACK >> (3u * cls)) & 7u);
  const bool rejected = (isbr && idf >= 5u) || (islu && idf >= 11u) || o3 < 3u;
  const bool isref = isbr || islu;
  off3 = isref ? (rejected ? 0xFFFFFFFFu : o3) : isl2 ? W + 3u : 0u;
  PlaceEnt e;
  e.cls = isref ? cls << 28 : 0u;
  e.ml = (islu || isl2) ? REC_K : 0u;
  e.mr = pfx == (uint32_t)P_RGB ? REC_K : (isref && rejected) ? EV_BAD : 0u;
  e.msd = pfx == (uint32_t)P_SMALL_DIFF ? 511u : 0u;
  return e;
}
// SMALL_DIFF index -> record constant (code.rs:230-247): index = rd + 7 gd + 49 bd
// (each difference + 3), constant = the three differences in spread form;
// entry 343 is 0 (what an event of another prefix reads)
struct alignas(16) SdlTable {
  uint32_t v[344];
};
constexpr SdlTable make_sdl_table() {
  SdlTable t{};
  for (uint32_t i = 0; i < 343u; ++i) {
    const uint32_t rd = i % 7u, t1 = i / 7u;
    t.v[i] = ((rd - 3u) & 255u) | ((((t1 % 7u) - 3u) & 255u) << 10) | ((((t1 / 7u) - 3u) & 255u) << 20);
  }
  return t;
}

// Both luma modes' constant in one sum over the three 10-bit lanes: with the
// event masked to its symbols (LUMA's reference out) and -16 / -32 / -16 added
// as 240 / 224 / 240, lane f1 is g = base - 32 (mod 256) and lanes f0 and f2
// get g added by one multiply; every lane sum is below 255 + 240 + 255 < 1024,
// so no carry crosses a lane, and REC_K drops what is above each byte.
constexpr uint32_t EV_LUMA_MASK = 0xFFu | (0x3Fu << 10) | (0xFFu << 20);
constexpr uint32_t EV_LUMA_K = 240u | (224u << 10) | (240u << 20);

// No position check can trip in a run of events whose first pixel is q0: the
// farthest reference is 3W + 3 back, and LUMA2 needs one row.
NICE_HDI bool place_deep(uint64_t q0, uint64_t W) { return q0 >= 3u * W + 3u; }

// make_record for dec_place, from the event word: 32-bit arithmetic (q <= N <=
// 2^30, 3W + 6 < 2^32).  sdl: make_sdl_table's 344 words; idt / off3: the
// PLACE_ENTRIES entries of place_entry.  CHECK: with the position checks (q is
// the pixel's index); without, q is not read -- only for events at or past a
// pixel that is place_deep.
template <bool CHECK>
NICE_HDI uint32_t place_record(uint32_t ev, uint32_t q, const uint32_t* sdl, const PlaceEnt* idt,
                               const uint32_t* off3, bool& bad) {
  // (a run event's bit 31 lands on the id field's low bit: any entry will do)
  const uint32_t entry = ((ev >> (EV_ID_SHIFT - 3u)) & 0x78u) | (ev >> EV_PFX_SHIFT);
  const PlaceEnt t = idt[entry];
  const uint32_t c_sd = sdl[(ev & t.msd) | (343u & ~t.msd)];
  const uint32_t lt = (ev & EV_LUMA_MASK) + EV_LUMA_K;
  const uint32_t x = lt + ((lt >> 10) & 255u) * 0x100001u;
  if (CHECK) bad = q + 3u < off3[entry];
  else bad = t.mr == EV_BAD;
  return t.cls | (x & t.ml) | (ev & t.mr) | c_sd;
}

}  // namespace nice
