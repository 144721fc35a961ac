// nice_rows.hpp -- the row kernels' spread-form arithmetic (nice_rows.hip):
// per-channel cyclic intervals, the per-pixel word kinds and the one-pixel
// steps.  No HIP header: a plain C++ compiler reads it too, so the CPU check of
// this arithmetic (tools/rows_arith_check.cpp, tests/test_rows_arith.py) runs
// the functions the kernels run.  The barrier kernels' body and its stages
// (unspread3_perm, the pre-passes) are nice_rows_body.hpp, which a host
// compiler reads through a shim of the HIP names; what needs DPP or wave votes
// stays in nice_rows.hip.
#pragma once
#include <stdint.h>

// host and device under hipcc (always inlined in a kernel), plain inline elsewhere
#if defined(__HIPCC__) || defined(__CUDACC__)
#define NICE_HDI __host__ __device__ __forceinline__
#else
#define NICE_HDI inline
#endif

namespace nice {

// Per-channel cyclic intervals [lo, lo+len] (mod 256) for the three channels
// in the "spread" layout (fields at bits 0, 10, 20 with two guard bits), so one
// 32-bit op acts on all channels.  An exact value is an interval with len 0;
// unknown is lo 0, len 255.  Rows are stored spread as well.
constexpr uint32_t SP_K = 0xFFu | (0xFFu << 10) | (0xFFu << 20);
constexpr uint32_t SP_K9 = 0x1FFu | (0x1FFu << 10) | (0x1FFu << 20);
constexpr uint32_t SP_1 = 1u | (1u << 10) | (1u << 20);
struct IvS { uint32_t lo, len; };
NICE_HDI uint32_t spread3(uint32_t v) {   // R | G<<8 | B<<16 -> spread
  return (v & 0xFFu) | ((v & 0xFF00u) << 2) | ((v & 0xFF0000u) << 4);
}
NICE_HDI uint32_t unspread3(uint32_t v) {
  return (v & 0xFFu) | ((v >> 2) & 0xFF00u) | ((v >> 4) & 0xFF0000u);
}
NICE_HDI IvS ivs_exact(uint32_t sp) { return IvS{sp, 0u}; }
NICE_HDI IvS ivs_add(IvS a, uint32_t c) { return IvS{(a.lo + c) & SP_K, a.len}; }
// floor((L + U) / 2) + c over an interval L: halves it unless it wraps past
// 255, in which case the hull of both halves is [U/2, (255+U)/2] -- the
// average of the whole range [0, 255], so a wrapping field is widened to that
// before the one averaging (instead of averaging both forms and selecting).
NICE_HDI IvS ivs_avg(IvS l, uint32_t u, uint32_t c) {
  const uint32_t s = l.lo + l.len;
  const uint32_t wm = ((s >> 8) & SP_1) * 0x3FFu;        // fields whose interval wraps
  const uint32_t lo0 = l.lo & ~wm, s0 = (s & ~wm) | (SP_K & wm);
  const uint32_t lo1 = ((lo0 + u) >> 1) & SP_K;
  const uint32_t hi1 = ((s0 + u) >> 1) & SP_K9;
  return IvS{(lo1 + c) & SP_K, hi1 - lo1};
}

// Per-pixel word: spread constant c in the field bits, the kind as one-hot
// flags in the guard bits -- W_L1/W_L2/W_L3: c plus the pixel 1..3 back;
// W_AVG: c plus floor((left + up) / 2); W_CUR: c plus one of pixels 0..2 of the
// current row (index in bits 8..9), unknown until lane 0 has them; none: the
// constant itself (a reference into a row above, already added).
constexpr uint32_t W_L1 = 1u << 28, W_AVG = 1u << 31, W_CUR = 1u << 18;   // W_L2, W_L3: bits 29, 30
// Kind bits >> 28 per record class, 4 bits per class: class 0 is the average
// (on row 0: the pixel to the left), classes 1-3 the pixel 1-3 back, classes
// 4-13 a pixel of a row above (no bits; W_CUR is added per pixel).
constexpr unsigned long long ROWS_KIND = (W_AVG >> 28) | ((unsigned long long)(W_L1 >> 28) << 4) |
                                         ((unsigned long long)((W_L1 << 1) >> 28) << 8) |
                                         ((unsigned long long)((W_L1 << 2) >> 28) << 12);
constexpr unsigned long long ROWS_KIND_Y0 = (ROWS_KIND & ~15ull) | (W_L1 >> 28);
static_assert((W_AVG >> 28) == 8u && (W_L1 >> 28) == 1u, "kind bits 28..31");
NICE_HDI uint32_t wmask(uint32_t w, int bit) {   // 0 or ~0
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_sbfe((int)w, bit, 1);
#else
  return 0u - ((w >> bit) & 1u);
#endif
}
// One pixel: kinds are selected with masks (no control flow, no SGPR masks).
// The constant is the word itself: its kind bits (18, 28..31) only reach a
// field's guard bits or bits >= 28 of the sums, which the masks after every
// add clear (no carry reaches a lower field: value bits <= 255 + 255 + 512).
// CUR = false: the caller knows no word holds W_CUR (waves without the row's
// last columns), two instructions fewer.
template <bool CUR = true>
NICE_HDI IvS rows_step(IvS l1, IvS l2, IvS l3, uint32_t u, uint32_t wp) {
  const uint32_t c = wp;
  const IvS va = ivs_avg(l1, u, c);
  const uint32_t m1 = wmask(wp, 28), m2 = wmask(wp, 29), m3 = wmask(wp, 30);
  const uint32_t ma = wmask(wp, 31);
  const uint32_t slo = (l1.lo & m1) | (l2.lo & m2) | (l3.lo & m3);
  const uint32_t slen = (l1.len & m1) | (l2.len & m2) | (l3.len & m3) | (CUR ? SP_K & wmask(wp, 18) : 0u);
  const uint32_t rlo = (slo + c) & SP_K;
  return IvS{(va.lo & ma) | (rlo & ~ma), (va.len & ma) | (slen & ~ma)};
}

// rows_chain when every input is exact (r0..r2 and the kept pixels): plain
// arithmetic, no intervals.  Only after the W_CUR words are resolved.
NICE_HDI uint32_t rows_step_exact(uint32_t l1, uint32_t l2, uint32_t l3, uint32_t u, uint32_t wp) {
  // (l1 + u) >> 1 leaves the next field's lowest bit in each guard bit 9:
  // with c (the word: no W_CUR bit once resolved) a field sums to <= 1022, so
  // one mask at the end clears both
  const uint32_t c = wp;
  // kinds as sign-extended bit masks: and / and-or / bit-insert selects, the
  // constant added once after the average-or-copy select (instead of compare
  // and select chains: one 4K frame reconstruct 9.02 -> 8.72 ms, 64 x 1080p
  // 4.10 -> 3.95, profiles/r05zr_ab_flow_steps.log)
  const uint32_t sel = (l1 & wmask(wp, 28)) | (l2 & wmask(wp, 29)) | (l3 & wmask(wp, 30));
  const uint32_t ma = (uint32_t)((int32_t)wp >> 31);
  const uint32_t x = (((l1 + u) >> 1) & ma) | (sel & ~ma);
  return (x + c) & SP_K;
}

}  // namespace nice
