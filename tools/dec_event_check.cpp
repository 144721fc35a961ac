// Host check of the decoder's event-word arithmetic: the functions of
// csrc/nice_dec_event.hpp themselves, which the kernels of nice_decode.hip
// compile too.  dec_place's record from an event word,
//   place_record(ev_pack(pfx, s0..s3), q)   with place_entry's tables for W,
// must equal dec_emit's record from the symbols, make_record(W, q, pfx,
// s0..s3) -- the record and the bad flag -- for every prefix, every symbol
// tuple of the payload streams' alphabets (stream_size; the 4-bit reference
// fields through 15, past the alphabets, for the ids the reference rejects),
// q in 0 .. 3W + 5 and one large q, W in {1, 2, 3, 4, 7, 64}.  The variant
// without position checks runs where the hoisting rule (place_deep) selects
// it, and is given a q it must not read.  The header is included by its path
// from this file, so a plain "g++ tools/dec_event_check.cpp" builds the check.
// Usage: dec_event_check   (exit 0: all equal)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../fast-losless-image-compression-format_amd/csrc/nice_dec_event.hpp"

using namespace nice;

namespace {
struct Tables {
  uint32_t W;
  PlaceEnt idt[PLACE_ENTRIES];
  uint32_t off3[PLACE_ENTRIES];
};
const SdlTable kSdl = make_sdl_table();
unsigned long long n_cases = 0, bad_rec = 0, bad_flag = 0, bad_word = 0;

// one (prefix, symbols) at every q of the list, both variants
inline void check(const Tables& T, const std::vector<uint32_t>& qs, uint32_t pfx, uint32_t s0, uint32_t s1,
                  uint32_t s2, uint32_t s3) {
  const uint32_t ev = ev_pack(pfx, s0, s1, s2, s3);
  if ((ev & EV_RUN) || (ev >> EV_PFX_SHIFT) != pfx) ++bad_word;
  for (uint32_t q : qs) {
    bool wbad, gbad;
    const uint32_t want = make_record(T.W, q, pfx, s0, s1, s2, s3, wbad);
    const uint32_t got = place_record<true>(ev, q, kSdl.v, T.idt, T.off3, gbad);
    bad_rec += got != want;
    bad_flag += gbad != wbad;
    ++n_cases;
    if (place_deep(q, T.W)) {
      const uint32_t got2 = place_record<false>(ev, 0xDEADBEEFu, kSdl.v, T.idt, T.off3, gbad);
      bad_rec += got2 != want;
      bad_flag += gbad != wbad;
      ++n_cases;
    }
  }
}
}  // namespace

int main() {
  const uint32_t Ws[] = {1, 2, 3, 4, 7, 64};
  for (uint32_t W : Ws) {
    Tables T;
    T.W = W;
    for (uint32_t e = 0; e < PLACE_ENTRIES; ++e) T.idt[e] = place_entry(e, W, T.off3[e]);
    std::vector<uint32_t> qs;
    for (uint32_t q = 0; q <= 3 * W + 5; ++q) qs.push_back(q);
    qs.push_back(1u << 29);
    for (uint32_t id = 0; id < 16; ++id) check(T, qs, P_BACK_REF, id, 0, 0, 0);
    for (uint32_t i = 0; i < (uint32_t)stream_size(S_SMALL_DIFF); ++i) check(T, qs, P_SMALL_DIFF, i, 0, 0, 0);
    for (uint32_t ref = 0; ref < 16; ++ref)
      for (uint32_t g = 0; g < (uint32_t)stream_size(S_LUMA_BASE); ++g)
        for (uint32_t r = 0; r < (uint32_t)stream_size(S_LUMA_OTHER); ++r)
          for (uint32_t b = 0; b < (uint32_t)stream_size(S_LUMA_OTHER); ++b) check(T, qs, P_LUMA, ref, g, r, b);
    for (uint32_t g = 0; g < (uint32_t)stream_size(S_LUMA2_BASE); ++g)
      for (uint32_t r = 0; r < (uint32_t)stream_size(S_LUMA2_R); ++r)
        for (uint32_t b = 0; b < (uint32_t)stream_size(S_LUMA2_B); ++b) check(T, qs, P_LUMA2, g, r, b, 0);
    for (uint32_t v = 0; v < (1u << 24); ++v) check(T, qs, P_RGB, v & 255u, (v >> 8) & 255u, v >> 16, 0);
  }
  printf("%llu cases: word %llu, record %llu, flag %llu mismatches\n", n_cases, bad_word, bad_rec, bad_flag);
  return (bad_word || bad_rec || bad_flag) ? 1 : 0;
}
