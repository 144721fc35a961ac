// nice_resize.hpp -- the integer arithmetic of the resized tensor output
// (include/nice.h, "image sets: resized tensor output"; the kernel is in
// nice_sets_resize.hip): where an output index samples its window axis, in
// 1/256 of a pixel, and the bilinear accumulator of four bytes; and, below, the
// tap ranges and weights of the antialiased reduction.  No HIP
// header: a plain C++ compiler reads it too, so the CPU check of this
// arithmetic (tools/resize_arith_check.cpp, tests/test_sets_resize_cpu.py)
// runs the functions the kernel runs.
#pragma once
#include <stdint.h>

// host and device under hipcc (always inlined in a kernel), plain inline elsewhere
#ifndef NICE_HDI
#if defined(__HIPCC__) || defined(__CUDACC__)
#define NICE_HDI __host__ __device__ __forceinline__
#else
#define NICE_HDI inline
#endif
#endif

namespace nice {

constexpr uint32_t RESIZE_MAX_OUT = 8192;   // the largest output axis

// Output index x of n_out over a window axis of n_in pixels (x < n_out <=
// RESIZE_MAX_OUT, 1 <= n_in <= 2^30): the taps i0 <= i1 < n_in and the weight
// f of i1 in 1/256 (i1 == i0 where f == 0).
struct ResizePos {
  uint32_t i0, i1, f;
};
NICE_HDI ResizePos resize_pos(uint32_t x, uint32_t n_in, uint32_t n_out) {
  // t: the nearest 1/256 (halves up) to (x + 1/2) * n_in / n_out; below 2^53
  const uint64_t num = (uint64_t)(2u * x + 1u) * n_in * 256u + n_out;
  const uint32_t den = 2u * n_out;
  // (the quotient of two numbers below 2^32 is the 32-bit division's)
  const uint64_t t = (num >> 32) == 0 ? (uint64_t)((uint32_t)num / den) : num / den;
  const uint64_t hi = (uint64_t)(n_in - 1u) * 256u;
  uint64_t q = t < 128u ? 0u : t - 128u;   // minus the half pixel, clamped to the window at 0 ...
  q = q < hi ? q : hi;                     // ... and at its last pixel
  const uint32_t i0 = (uint32_t)(q >> 8), f = (uint32_t)(q & 255u);
  const uint32_t i1 = (f != 0 && i0 + 1u < n_in) ? i0 + 1u : i0;
  return ResizePos{i0, i1, f};
}

// The bilinear sum of four bytes, row j0 then row j1, in 1/65536: at most
// 255 * 65536 < 2^24, so binary32 holds it exactly.
NICE_HDI uint32_t resize_acc(uint32_t b00, uint32_t b01, uint32_t b10, uint32_t b11, uint32_t fx, uint32_t fy) {
  return (256u - fy) * ((256u - fx) * b00 + fx * b01) + fy * ((256u - fx) * b10 + fx * b11);
}

// acc / 65536 in binary32: exact (no rounding in the conversion or the scaling).
NICE_HDI float resize_unit(uint32_t acc) { return (float)acc * 0x1p-16f; }

// ---- antialiased reduction (include/nice.h, "image sets: antialiased resized
// tensor output"; the kernels are in nice_sets_resize_aa.hip) ------------------
// The triangle filter of support n_in / n_out over a reducing axis (n_out <
// n_in <= RESIZE_AA_MAX_IN, n_out <= RESIZE_MAX_OUT), in integers: with
// C = (2x + 1) * n_in, P_i = (2i + 1) * n_out and S = 2 * n_in (all below 2^30)
// pixel i has the raw weight r_i = S - |P_i - C| where that is positive, and
// the weight w_i = W_i - W_(i-1) in 1/4096, W_i = (cum_i * 8192 + R) / (2 R).
constexpr uint32_t RESIZE_AA_MAX_IN = 65536;   // the longest reducing axis

// An axis the antialiased entry points take: it does not reduce, or fits the limit.
NICE_HDI bool resize_aa_axis_ok(uint32_t n_in, uint32_t n_out) { return n_out >= n_in || n_in <= RESIZE_AA_MAX_IN; }

// The weights of the two taps of a non-reducing axis (resize_pos), in 1/4096.
NICE_HDI uint32_t resize_aa_w0(uint32_t f) { return 16u * (256u - f); }
NICE_HDI uint32_t resize_aa_w1(uint32_t f) { return 16u * f; }

// The taps lo..hi of output index x: the i with r_i > 0, inside the window.
struct ResizeAaRange {
  uint32_t lo, hi;
};
NICE_HDI ResizeAaRange resize_aa_range(uint32_t x, uint32_t n_in, uint32_t n_out) {
  const uint32_t C = (2u * x + 1u) * n_in, S = 2u * n_in;
  // lo: the first i with (2i + 1) * n_out > C - S;  hi: the last with (2i + 1) * n_out < C + S
  const uint32_t lo = C > S ? ((C - S) / n_out + 1u) >> 1 : 0u;
  const uint32_t k = (C + S - 1u) / n_out;   // >= 3
  const uint32_t hi = (k - 1u) >> 1;
  return ResizeAaRange{lo, hi < n_in - 1u ? hi : n_in - 1u};
}

// r_i of output index x (lo <= i <= hi: positive).
NICE_HDI uint32_t resize_aa_raw(uint32_t i, uint32_t x, uint32_t n_in, uint32_t n_out) {
  const uint32_t C = (2u * x + 1u) * n_in, P = (2u * i + 1u) * n_out;
  return 2u * n_in - (P > C ? P - C : C - P);
}

// cum_i = r_lo + ... + r_i (lo <= i <= hi), by the closed form of two
// arithmetic series: r rises by 2 n_out per pixel up to the last pixel m with
// P_m <= C and falls by as much after it.  Below 2^34; the terms below 2^50.
NICE_HDI uint64_t resize_aa_cum(uint32_t i, uint32_t lo, uint32_t x, uint32_t n_in, uint32_t n_out) {
  const int64_t C = (int64_t)((2u * x + 1u) * n_in), S = 2 * (int64_t)n_in;
  const uint32_t m = ((2u * x + 1u) * n_in / n_out - 1u) >> 1;   // lo <= m <= hi
  const uint32_t a = i < m ? i : m;
  // the sum of 2k + 1 over k = p .. q is (q + 1)^2 - p^2
  int64_t cum = (int64_t)(a - lo + 1u) * (S - C) + (int64_t)n_out * ((int64_t)(a + 1u) * (a + 1u) - (int64_t)lo * lo);
  if (i > m) cum += (int64_t)(i - m) * (S + C) - (int64_t)n_out * ((int64_t)(i + 1u) * (i + 1u) - (int64_t)(m + 1u) * (m + 1u));
  return (uint64_t)cum;
}

// W = (cum * 8192 + R) / (2 R), cum <= R: the nearest 1/4096 to cum / R, halves up.
NICE_HDI uint32_t resize_aa_W(uint64_t cum, uint64_t R) {
  // (R below 2^18: the numerator is below 2^32 and the division the 32-bit one)
  if ((R >> 18) == 0) return ((uint32_t)cum * 8192u + (uint32_t)R) / (2u * (uint32_t)R);
  return (uint32_t)((cum * 8192u + R) / (2u * R));
}

// w_i of output index x, whose taps are lo..hi and whose R is resize_aa_cum(hi, ...).
NICE_HDI uint32_t resize_aa_weight(uint32_t i, uint32_t lo, uint64_t R, uint32_t x, uint32_t n_in, uint32_t n_out) {
  const uint64_t cum = resize_aa_cum(i, lo, x, n_in, n_out);
  const uint32_t W = resize_aa_W(cum, R);
  return i > lo ? W - resize_aa_W(cum - resize_aa_raw(i, x, n_in, n_out), R) : W;
}

// The sum of row weights times row sums, in 1/2^24, to the accumulator in
// 1/65536: at most 255 * 65536, which resize_unit takes.
NICE_HDI uint32_t resize_aa_round(uint32_t acc32) { return (acc32 + 128u) >> 8; }

}  // namespace nice
