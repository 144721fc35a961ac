// nice_dec_state.hpp -- the packed state words the decoder's parse kernels
// exchange (slice entry, `last`, checkpoint) and the pixel arithmetic of a
// parse, one accessor each.  No HIP header: a plain C++ compiler reads it too,
// so the CPU check (tools/dec_state_check.cpp, tests/test_dec_state_arith.py)
// runs the functions the kernels of nice_decode.hip run.
#pragma once
#include <stdint.h>

#include "nice_format.h"

namespace nice {

// Run digits read in the current run (dk): 0 outside a run, then 1..64.
constexpr uint32_t DK_BITS = 7, DK_MASK = (1u << DK_BITS) - 1u;

// ---- slice entry: bit position relative to the data start, run digits ------
constexpr uint32_t PS_POS_BITS = 40, PS_DK_SHIFT = 44;
constexpr unsigned long long PS_MASK = (1ull << (PS_DK_SHIFT + DK_BITS)) - 1ull;
static_assert(PS_POS_BITS <= PS_DK_SHIFT, "entry: the position ends below the run digits");
NICE_HDI unsigned long long ps_pack(unsigned long long rel, uint32_t dk) {
  return rel | ((unsigned long long)dk << PS_DK_SHIFT);
}
NICE_HDI unsigned long long ps_pos(unsigned long long e) { return e & ((1ull << PS_POS_BITS) - 1ull); }
NICE_HDI uint32_t ps_dk(unsigned long long e) { return (uint32_t)(e >> PS_DK_SHIFT) & DK_MASK; }

// ---- `last`: the entry a slice was last parsed from, and in bits 56..63 the
// number of valid checkpoints that parse left; LAST_NEVER before any parse.
// (An entry's bits 40..43 are 0, so LAST_NEVER equals no entry.)
constexpr uint32_t LAST_NCK_SHIFT = 56;
constexpr unsigned long long LAST_NEVER = ~0ull;
static_assert(PS_DK_SHIFT + DK_BITS <= LAST_NCK_SHIFT, "last: the entry ends below the checkpoint count");
NICE_HDI unsigned long long last_pack(unsigned long long e, uint32_t n_ck) {
  return e | ((unsigned long long)n_ck << LAST_NCK_SHIFT);
}
NICE_HDI uint32_t last_nck(unsigned long long last) { return (uint32_t)(last >> LAST_NCK_SHIFT); }
NICE_HDI bool last_never(unsigned long long last) { return last == LAST_NEVER; }
NICE_HDI bool last_from(unsigned long long last, unsigned long long e) { return (last & PS_MASK) == e; }

// ---- checkpoint: position in the slice, run digits, pixels since the entry.
// The low word is the key a re-parse compares with the previous parse's.
constexpr uint32_t CK_POS_BITS = 16, CK_DK_SHIFT = 20, CK_PX_SHIFT = 32;
static_assert(CK_POS_BITS <= CK_DK_SHIFT && CK_DK_SHIFT + DK_BITS <= CK_PX_SHIFT, "checkpoint fields");
NICE_HDI uint32_t ck_key(uint32_t pos, uint32_t dk) { return pos | (dk << CK_DK_SHIFT); }
NICE_HDI unsigned long long ck_pack(uint32_t key, uint32_t px) {
  return key | ((unsigned long long)px << CK_PX_SHIFT);
}
NICE_HDI uint32_t ck_key_of(unsigned long long c) { return (uint32_t)c; }
NICE_HDI uint32_t ck_pos(unsigned long long c) { return (uint32_t)c & ((1u << CK_POS_BITS) - 1u); }
NICE_HDI uint32_t ck_dk(unsigned long long c) { return (uint32_t)(c >> CK_DK_SHIFT) & DK_MASK; }
NICE_HDI uint32_t ck_px(unsigned long long c) { return (uint32_t)(c >> CK_PX_SHIFT); }
// the same checkpoint of a parse that counted delta pixels more (mod 2^32) before it
NICE_HDI unsigned long long ck_add_px(unsigned long long c, uint32_t delta) {
  return ck_pack(ck_key_of(c), ck_px(c) + delta);
}

// ---- pixel arithmetic ------------------------------------------------------
// Pixels a prefix accounts for: 1 for a coded pixel; a run digit d contributes
// d << 3k (k = digits read before it; the reference's u8 shift counter `+= 3`
// only matters mod 64) plus the run's first pixel on its first digit
// (code.rs:660-680).  dk: digits read in the current run, kept in 1..64 once
// nonzero.  Saturates at 2^32 - 1 (only garbage parses get there).  (In 64
// bits throughout: dec_sync's step had a 32-bit shift below 2^30 first, and
// is 2-4 % faster without it.)
NICE_HDI uint32_t pixel_count(uint32_t pfx, uint32_t& dk) {
  if (pfx < (uint32_t)P_RUN1) { dk = 0; return 1u; }
  const uint32_t sh = (3u * dk) & 63u;
  const uint64_t c = ((uint64_t)(pfx - P_RUN1) << sh) + (dk == 0 ? 1u : 0u);
  dk = dk >= 64u ? 1u : dk + 1u;
  return c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c;
}
NICE_HDI uint32_t sat_add(uint32_t a, uint32_t b) { return a + b < a ? 0xFFFFFFFFu : a + b; }

}  // namespace nice
