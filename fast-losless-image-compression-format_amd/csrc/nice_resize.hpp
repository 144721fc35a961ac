// nice_resize.hpp -- the integer arithmetic of the resized tensor output
// (include/nice.h, "image sets: resized tensor output"; the kernel is in
// nice_sets_resize.hip): where an output index samples its window axis, in
// 1/256 of a pixel, and the bilinear accumulator of four bytes.  No HIP
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

}  // namespace nice
