// hip/hip_runtime.h of tools/hip_host_shim -- the HIP names that
// csrc/nice_rows_body.hpp (and the headers it includes) use, for a plain C++20
// compiler: one workgroup as host threads, one std::barrier as the block
// barrier, LDS and device memory as heap buffers that a sanitizer can watch.
// Only tools/rows_host_check.cpp uses it (g++ -I tools/hip_host_shim); it is
// no HIP implementation: what the row body does not use is missing or aborts.
#pragma once
// glibc declares nice(int); the project's namespace is nice.  The system
// headers are read once, here, with that function renamed.
#define nice glibc_nice
#include <unistd.h>

#include <algorithm>
#include <barrier>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#undef nice

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __shared__ static   // one copy per block: the host runs one block at a time
#define __launch_bounds__(...)

struct hip_host_dim3 { uint32_t x, y, z; };
struct uint2 { uint32_t x, y; };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
using std::max;
using std::min;

inline thread_local hip_host_dim3 threadIdx{0, 0, 0};
inline hip_host_dim3 blockIdx{0, 0, 0}, blockDim{1, 1, 1};

namespace hip_host_shim {

inline void* dyn_lds = nullptr;                  // the block's dynamic LDS (NICE_ROWS_DYN_LDS)
inline std::barrier<>* block_barrier = nullptr;  // every launched thread arrives, as on the device
inline void barrier() { block_barrier->arrive_and_wait(); }
[[noreturn]] inline void missing(const char* what) {
  std::fprintf(stderr, "hip_host_shim: %s has no host form\n", what);
  std::abort();
}
// v_perm_b32: byte i of the result is byte sel[i] of {hi, lo} (0..3: lo, 4..7:
// hi), 0x0C: 0x00, 0x0D and above: 0xFF; the sign-replicating selectors 8..11
// are not used by the row kernels
inline uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
  const uint64_t src = (uint64_t)hi << 32 | lo;
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t s = (sel >> (8 * i)) & 0xFFu;
    if (s >= 8 && s < 12) missing("v_perm_b32 selectors 8..11");
    const uint32_t b = s < 8 ? (uint32_t)(src >> (8 * s)) & 0xFFu : s == 12 ? 0u : 0xFFu;
    r |= b << (8 * i);
  }
  return r;
}
inline int no_dpp(int, int, int, int, int, bool) { missing("DPP"); }

// One block of `threads` host threads through kernel(args); lds: its dynamic LDS.
template <class Kernel, class Args>
void launch(Kernel kernel, const Args& args, uint32_t threads, void* lds) {
  std::barrier<> bar((std::ptrdiff_t)threads);
  block_barrier = &bar;
  dyn_lds = lds;
  blockDim = hip_host_dim3{threads, 1, 1};
  blockIdx = hip_host_dim3{0, 0, 0};
  std::vector<std::thread> pool;
  pool.reserve(threads);
  for (uint32_t t = 0; t < threads; ++t)
    pool.emplace_back([&, t] {
      threadIdx = hip_host_dim3{t, 0, 0};
      kernel(args);
    });
  for (auto& th : pool) th.join();
  block_barrier = nullptr;
  dyn_lds = nullptr;
}

}  // namespace hip_host_shim

inline void __syncthreads() { hip_host_shim::barrier(); }
// s_barrier and its LDS fences: the one host barrier orders everything
#define __builtin_amdgcn_s_barrier() hip_host_shim::barrier()
#define __builtin_amdgcn_fence(...) ((void)0)
#define __builtin_amdgcn_s_memtime() 0ull
#define __builtin_amdgcn_perm(hi, lo, sel) hip_host_shim::perm((hi), (lo), (sel))
#define __builtin_amdgcn_update_dpp(...) hip_host_shim::no_dpp(__VA_ARGS__)
inline uint32_t __umul24(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
inline int __any(int) { hip_host_shim::missing("a wave vote (__any)"); }

inline uint32_t atomicOr(uint32_t* p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
inline int atomicCAS(int* p, int expected, int v) {
  __atomic_compare_exchange_n(p, &expected, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
  return expected;
}
inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) {
  return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST);
}
