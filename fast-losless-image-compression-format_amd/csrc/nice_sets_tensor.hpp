// nice_sets_tensor.hpp -- what the tensor merges share (nice_sets_tensor.hip,
// nice_sets_resize.hip, nice_sets_resize_aa.hip), each stage once: the value
// and the stored form of an element, the stores of a lane's group of elements,
// the source of a slot position, values pinned to vector registers, and the
// dtype x layout ladder of the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/nice.h"
#include "nice_slot_plan.hpp"
#include "nice_tiles.hpp"

namespace nice {

// The stored form of an element: its bits, from the binary32 value.
template <int DT> struct TensorElem;
template <> struct TensorElem<(int)NICE_TENSOR_F32> {
  using bits = uint32_t;
  static __device__ __forceinline__ bits cvt(float v) { return __float_as_uint(v); }
};
template <> struct TensorElem<(int)NICE_TENSOR_F16> {
  using bits = uint16_t;
  static __device__ __forceinline__ bits cvt(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }
};
template <> struct TensorElem<(int)NICE_TENSOR_BF16> {
  using bits = uint16_t;
  static __device__ __forceinline__ bits cvt(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }
};

// The element of include/nice.h, and the only place one is made: v = fmaf(x,
// scale, bias) rounded to binary32, then v rounded to nearest even to the type
// -- two roundings for a 16-bit type.  The empty asm keeps the compiler from
// fusing both into v_fma_mixlo_f16 / v_fma_mixhi_f16, which round the exact
// sum once, to binary16 (gfx950 has no such instruction for bfloat16, and
// float32 is not rounded again: they need no fence and get none).
template <int DT>
__device__ __forceinline__ typename TensorElem<DT>::bits tensor_value(float x, float scale, float bias) {
  float v = __fmaf_rn(x, scale, bias);
  if constexpr (DT == (int)NICE_TENSOR_F16) asm("" : "+v"(v));
  return TensorElem<DT>::cvt(v);
}

// P elements at p (aligned to their P * sizeof(B) bytes) as one store.
template <typename B, uint32_t P>
__device__ __forceinline__ void st_elems(B* p, const B* e) {
  constexpr uint32_t W = P * sizeof(B) / 4;
  static_assert(W == 1 || W == 2 || W == 4, "a store of 4, 8 or 16 bytes");
  uint32_t w[W];
#pragma unroll
  for (uint32_t i = 0; i < W; ++i) {
    if constexpr (sizeof(B) == 4) w[i] = e[i];
    else w[i] = (uint32_t)e[2 * i] | ((uint32_t)e[2 * i + 1] << 16);
  }
  if constexpr (W == 1) *reinterpret_cast<uint32_t*>(p) = w[0];
  else if constexpr (W == 2) *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
  else *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}

// The group of P > 1 output columns at xo (a multiple of P) of the row at
// orow, elem(k, c) being channel c of column xo + k: planar, P elements per
// plane as one store; interleaved, the 3 P elements as three.
template <typename B, uint32_t P, int LAYOUT, class Elem>
__device__ __forceinline__ void st_group(B* orow, uint64_t plane_pitch, uint32_t xo, Elem elem) {
  if (LAYOUT == (int)NICE_TENSOR_PLANAR) {
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
      B e[P];
#pragma unroll
      for (uint32_t k = 0; k < P; ++k) e[k] = elem(k, c);
      st_elems<B, P>(orow + c * plane_pitch + xo, e);
    }
  } else {
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {   // third c of the 3 P elements: element j is channel j % 3 of column j / 3
      B e[P];
#pragma unroll
      for (uint32_t k = 0; k < P; ++k) e[k] = elem((c * P + k) / 3u, (c * P + k) % 3u);
      st_elems<B, P>(orow + 3ull * xo + c * P, e);
    }
  }
}
// Output column xo alone, element by element; elem(c) is its channel c.
template <typename B, int LAYOUT, class Elem>
__device__ __forceinline__ void st_one(B* orow, uint64_t plane_pitch, uint32_t xo, Elem elem) {
#pragma unroll
  for (uint32_t c = 0; c < 3; ++c) {
    const B e = elem(c);
    if (LAYOUT == (int)NICE_TENSOR_PLANAR) orow[c * plane_pitch + xo] = e;
    else orow[3ull * xo + c] = e;
  }
}

// Where the pixels of slot position p are (src: slot_position_sources; status
// may be null): pixel i of the slot at base + i * bpp; bpp 0: nothing to read
// there (a failed or refused slot).
struct SlotSource {
  const uint8_t* base;
  uint32_t bpp;
};
__device__ __forceinline__ SlotSource slot_source(const unsigned long long* src, const int32_t* status, const uint8_t* tiles,
                                                  uint64_t tile_stride, const uint8_t* packed, uint32_t p) {
  const uint64_t s = src[p];
  const uint32_t kind = (uint32_t)(s >> 62);
  const uint64_t v = s & SLOT_SRC_VALUE;
  const bool bad = kind > 1u || (status && status[p] != 0);
  const uint8_t* base = kind == 0u ? tiles + v * tile_stride : packed + v;
  return SlotSource{base, bad ? 0u : kind == 0u ? 4u : 3u};
}
// bytes +0..+2 of pixel i (bpp != 0): one dword of a dense slot, three bytes of a raw one
__device__ __forceinline__ uint32_t ld_tap(const SlotSource& s, uint32_t i) {
  const uint8_t* p = s.base + (uint64_t)i * s.bpp;
  return s.bpp == 4u ? ld32(p) : ld_px_bytes(p, 3u, 0u);
}

// x, held in a vector register: a constant that is the same in every lane, or
// an address the lanes add to, kept out of the scalar registers, which are
// short (the window, the arguments and the loops' masks and bounds fill them)
template <class T>
__device__ __forceinline__ T in_vgpr(T x) {
  static_assert(sizeof(T) == 4, "one register");
  asm("" : "+v"(x));
  return x;
}
__device__ __forceinline__ uint64_t in_vgpr64(uint64_t x) {
  return ((uint64_t)in_vgpr((uint32_t)(x >> 32)) << 32) | in_vgpr((uint32_t)x);
}

// The one dtype x layout ladder: f(dt, layout), two std::integral_constant<int>
// that name the kernel's instantiation, launches it.  NICE_E_ARG for a dtype
// that is none of the three (the layout is the caller's to have checked:
// set_tensor_check).
template <class F>
int tensor_dispatch(uint32_t dtype, uint32_t layout, F f) {
  const auto with = [&](auto dt) {
    if (layout == NICE_TENSOR_PLANAR) f(dt, std::integral_constant<int, (int)NICE_TENSOR_PLANAR>{});
    else f(dt, std::integral_constant<int, (int)NICE_TENSOR_INTERLEAVED>{});
    return (int)NICE_OK;
  };
  if (dtype == NICE_TENSOR_F32) return with(std::integral_constant<int, (int)NICE_TENSOR_F32>{});
  if (dtype == NICE_TENSOR_F16) return with(std::integral_constant<int, (int)NICE_TENSOR_F16>{});
  if (dtype == NICE_TENSOR_BF16) return with(std::integral_constant<int, (int)NICE_TENSOR_BF16>{});
  return NICE_E_ARG;
}

}  // namespace nice
