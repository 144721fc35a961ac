// Host check of the decoder's packed state words and pixel arithmetic: the
// functions of csrc/nice_dec_state.hpp themselves, which the kernels of
// nice_decode.hip compile too.
//  * pixel_count against the 64-bit formula written out here as the
//    specification, for every prefix of the prefix alphabet x dk in 0..64: the
//    count and the next dk;
//  * every pack / unpack round trip of the slice entry, `last` and the
//    checkpoint at the field limits, ck_add_px's wrap, sat_add.
// The header is included by its path from this file, so a plain
// "g++ tools/dec_state_check.cpp" builds the check.
// Usage: dec_state_check   (exit 0: all equal)
#include <cstdint>
#include <cstdio>

#include "../fast-losless-image-compression-format_amd/csrc/nice_dec_state.hpp"

using namespace nice;

namespace {
unsigned long long n_cases = 0, bad_count = 0, bad_word = 0;

// the specification: code.rs:660-680 in 64 bits, saturated to 32
uint32_t spec_pixel_count(uint32_t pfx, uint32_t& dk) {
  if (pfx < (uint32_t)P_RUN1) { dk = 0; return 1u; }
  const uint32_t sh = (3u * dk) & 63u;
  const uint64_t c = ((uint64_t)(pfx - P_RUN1) << sh) + (dk == 0 ? 1u : 0u);
  dk = dk >= 64u ? 1u : dk + 1u;
  return c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c;
}
// (The header's pixel_count is this formula too; the two are kept as texts of
// their own, so an edit of the header is held against this one.)
// A second formulation, the one dec_sync's step ran before there was one
// pixel_count: a 32-bit shift below 2^30 (d <= 7 fits), 64 bits from there.
uint32_t step_pixel_count(uint32_t pfx, uint32_t& dk) {
  if (pfx < (uint32_t)P_RUN1) { dk = 0; return 1u; }
  const uint32_t sh = (3u * dk) & 63u, d = pfx - (uint32_t)P_RUN1;
  uint32_t c;
  if (sh < 30u) {
    c = (d << sh) + (dk == 0 ? 1u : 0u);
  } else {
    const uint64_t c64 = (uint64_t)d << sh;
    c = c64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c64;
  }
  dk = dk >= 64u ? 1u : dk + 1u;
  return c;
}
void expect(bool ok) {
  ++n_cases;
  bad_word += ok ? 0 : 1;
}
}  // namespace

int main() {
  for (uint32_t pfx = 0; pfx < (uint32_t)stream_size(S_PREFIX); ++pfx)
    for (uint32_t dk = 0; dk <= 64u; ++dk) {
      uint32_t dw = dk, dg = dk, ds = dk;
      const uint32_t want = spec_pixel_count(pfx, dw), got = pixel_count(pfx, dg);
      const uint32_t was = step_pixel_count(pfx, ds);
      bad_count += (got != want || dg != dw || was != want || ds != dw) ? 1 : 0;
      ++n_cases;
    }
  const uint32_t dks[] = {0u, 1u, 63u, 64u, DK_MASK};
  const unsigned long long rels[] = {0ull, 1ull, 1ull << 39, (1ull << PS_POS_BITS) - 1ull};
  const uint32_t ncks[] = {0u, 1u, 254u, 255u};
  for (unsigned long long rel : rels)
    for (uint32_t dk : dks) {
      const unsigned long long e = ps_pack(rel, dk);
      expect(ps_pos(e) == rel && ps_dk(e) == dk && (e & PS_MASK) == e);
      expect(!last_never(e) && !last_from(LAST_NEVER, e));
      for (uint32_t n : ncks) {
        const unsigned long long last = last_pack(e, n);
        expect(last_nck(last) == n && last_from(last, e) && !last_never(last));
        expect(!last_from(last, ps_pack(rel ^ 1ull, dk)) && !last_from(last, ps_pack(rel, dk ^ 1u)));
      }
    }
  const uint32_t poss[] = {0u, 1u, 0x8000u, (1u << CK_POS_BITS) - 1u};
  const uint32_t pxs[] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu};
  for (uint32_t pos : poss)
    for (uint32_t dk : dks)
      for (uint32_t px : pxs) {
        const uint32_t key = ck_key(pos, dk);
        const unsigned long long c = ck_pack(key, px);
        expect(ck_key_of(c) == key && ck_pos(c) == pos && ck_dk(c) == dk && ck_px(c) == px);
        expect(ck_key(pos ^ 1u, dk) != key && ck_key(pos, dk ^ 1u) != key);
        for (uint32_t delta : pxs) {
          const unsigned long long d = ck_add_px(c, delta);
          expect(ck_key_of(d) == key && ck_px(d) == px + delta);   // (mod 2^32)
        }
        for (uint32_t b : pxs) {
          const uint64_t s = (uint64_t)px + b;
          expect(sat_add(px, b) == (s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s));
        }
      }
  printf("%llu cases: count %llu, word %llu mismatches\n", n_cases, bad_count, bad_word);
  return (bad_count || bad_word) ? 1 : 0;
}
