// nice_pack.hpp -- the pack kernels' integer arithmetic (nice_pack.hip): a
// tile's extent, the base-8 run digits and their table index, the run after a
// pixel from a word of coded flags, where a span of bits lands in the stream's
// 32-bit words, and the window arithmetic of a wrapped write.  No HIP header: a
// plain C++ compiler reads it too, so the CPU check of this arithmetic
// (tools/pack_arith_check.cpp, tests/test_pack_arith.py) runs the functions the
// kernels run.  What loads, stores or needs a wave stays in nice_pack.hip.
#pragma once
#include <stdint.h>

#include "nice_geom.h"   // (NICE_HDI)

namespace nice {

// run digits (prefixes 5..12, code.rs:391-406) after a coded pixel, m = run - 1:
// entries 0..63 the natural digits of m, 64 + x the two digits (x & 7, x >> 3)
// of a longer run's first two, 128 no run
constexpr uint32_t RC_TWO = 64, RC_NONE = 128, RC_N = 130;

// Tile tt of a frame of N pixels: its first pixel and its pixel count (the
// last tile may be partial).
struct TileExtent {
  int64_t start;
  int count;
};
NICE_HDI TileExtent pack_tile_extent(int64_t N, uint32_t tt) {
  const int64_t start = (int64_t)tt * ENC_TILE;
  return TileExtent{start, (int)((N - start) < ENC_TILE ? (N - start) : ENC_TILE)};
}

// fn(d) for every base-8 digit d of run - 1, low digit first, at least one: the
// digits after a coded pixel with `run` >= 1 repeats (code.rs:391-406).
template <class Fn>
NICE_HDI void pack_run_digits(uint32_t run, Fn&& fn) {
  uint32_t m = run - 1u;
  while (true) {
    fn(m & 7u);
    if (m < 8) break;
    m >>= 3;
  }
}
// The digits past the first two, which the table entry rc_index(run) holds:
// none unless run > 64, else the digits of (run - 1) >> 6.
template <class Fn>
NICE_HDI void pack_run_digits_past2(uint32_t run, Fn&& fn) {
  if (run > 64u) pack_run_digits(((run - 1u) >> 6) + 1u, fn);
}
// PackTab::rc entry of a run: its one or two first digits (run == 0: no run).
NICE_HDI uint32_t rc_index(uint32_t run) {
  const uint32_t m = run - 1u;
  return run == 0 ? RC_NONE : m < 64u ? m : RC_TWO + (m & 63u);
}

// Run after pixel q of a thread's pixels (0 for run members).  flags: their
// coded flags, bit q for pixel q (4 or 16 pixels); s: the first one's index;
// after: the first coded pixel past them.
NICE_HDI uint32_t pack_run_after(uint32_t flags, int q, uint32_t s, uint32_t after) {
  const uint32_t later = flags >> (q + 1);
  const uint32_t nxt = later ? s + (uint32_t)(q + 1) + (uint32_t)__builtin_ctz(later) : after;
  return ((flags >> q) & 1u) ? nxt - (s + (uint32_t)q) - 1u : 0u;
}

// `bits` stream bits from bit s0 on, in 32-bit words: they reach words w0 ..
// w0 + nw - 1, the first of them at bit sh of word w0.  Word 0 is shared with
// what precedes the span when sh != 0, word nw - 1 with what follows it when
// the span ends inside it.
struct BitSpan {
  uint64_t w0;
  uint32_t sh, nw, eh;   // eh: the end bit within its word
};
NICE_HDI BitSpan pack_span(uint64_t s0, uint32_t bits) {
  const uint64_t e0 = s0 + bits;
  const uint32_t sh = (uint32_t)(s0 & 31);
  const uint64_t w0 = s0 >> 5;
  const uint32_t nw = bits ? (uint32_t)(((e0 + 31) >> 5) - w0) : 0u;
  return BitSpan{w0, sh, nw, (uint32_t)(e0 & 31)};
}
NICE_HDI bool pack_span_first_shared(BitSpan sp, uint32_t m) { return m == 0 && sp.sh; }
NICE_HDI bool pack_span_last_shared(BitSpan sp, uint32_t m) { return m == sp.nw - 1 && sp.eh; }

// The reference's write_24bits (bitwriter.rs:55-73) of an n-bit code v with
// bo = bit_offset pending bits when bo + n > 32: `32 - bit_offset` wraps (u8),
// the shift is masked to 5 bits and the code is added into the cache.  w: the
// 32-bit window at the pending bits' byte (big-endian); returns its new value.
NICE_HDI uint32_t pack_wrapped_window(uint32_t w, uint32_t bo, uint32_t v, uint32_t n) {
  const uint32_t sh = (uint32_t)(uint8_t)(32u - (uint8_t)(bo + n)) & 31u;
  return w + (v << sh);
}

}  // namespace nice
