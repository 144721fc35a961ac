// nice_sets_tensor.hpp -- what the tensor merges share (nice_sets_tensor.hip,
// nice_sets_resize.hip, nice_sets_resize_aa.hip): the stored form of an element and the combined store
// of a lane's consecutive elements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nice.h"

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

}  // namespace nice
