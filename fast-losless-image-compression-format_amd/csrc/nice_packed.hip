// nice_packed.hip -- packed stream batches (include/nice.h, "Packed stream
// batches"): the offset scan and the ragged copy that compacts a strided batch
// of streams into one buffer.  The host knows no stream length: both kernels
// take them from device memory, and the copy sizes its work from off[n].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/nice.h"
#include "nice_kernels.h"
#include "nice_internal.h"

namespace nice {

constexpr uint32_t PK_SCAN_THREADS = 1024;
constexpr uint32_t PK_COPY_THREADS = 256;
constexpr uint32_t PK_COPY_BLOCKS_PER_CU = 4;   // 16 waves per CU, each with 4 x 1 KiB of loads in flight
constexpr uint32_t PK_UNROLL = 4;

// Inclusive wave64 prefix sum of 63-bit values: three 21-bit digits through the
// 32-bit DPP scan (64 x 2^21 fits a digit's sum), recombined.
__device__ __forceinline__ unsigned long long wave_incl_scan64(unsigned long long v) {
  const unsigned long long a = wave_incl_scan((uint32_t)v & 0x1FFFFFu);
  const unsigned long long b = wave_incl_scan((uint32_t)(v >> 21) & 0x1FFFFFu);
  const unsigned long long c = wave_incl_scan((uint32_t)(v >> 42) & 0x1FFFFFu);
  return a + (b << 21) + (c << 42);
}

// off[0] = 0, off[f + 1] = off[f] + align16(len[f]); one block, pieces of
// PK_SCAN_THREADS lengths with a carry.  A length above the stride (the slot
// cannot hold it) counts as 0 and makes the status NICE_E_ARG; else the status
// says whether off[n] fits the capacity.
__global__ __launch_bounds__(PK_SCAN_THREADS) void pack_scan(const unsigned long long* __restrict__ len,
                                                             uint64_t stride, uint32_t n,
                                                             unsigned long long* __restrict__ off,
                                                             unsigned long long cap, int32_t* status) {
  __shared__ unsigned long long wsum[PK_SCAN_THREADS / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long carry = 0;   // granules before this piece
  bool over = false;
  if (threadIdx.x == 0) off[0] = 0;
  for (uint64_t base = 0; base < n; base += PK_SCAN_THREADS) {
    const uint64_t i = base + threadIdx.x;
    unsigned long long g = 0;
    if (i < n) {
      const unsigned long long l = len[i];
      if (l > stride) over = true;
      else g = (l >> 4) + ((l & 15u) != 0);
    }
    const unsigned long long incl = wave_incl_scan64(g);
    if (lane == 63u) wsum[wave] = incl;
    __syncthreads();
    unsigned long long pre = carry, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < PK_SCAN_THREADS / 64; ++w) {
      const unsigned long long s = wsum[w];
      pre += w < wave ? s : 0ull;
      tot += s;
    }
    if (i < n) off[i + 1] = (pre + incl) << 4;
    carry += tot;
    __syncthreads();
  }
  const int any_over = __syncthreads_or(over ? 1 : 0);
  if (threadIdx.x == 0) *status = any_over ? NICE_E_ARG : (carry << 4) > cap ? NICE_E_CAPACITY : NICE_OK;
}

// Word w (0..3) of a granule that holds r valid bytes: all ones where the
// bytes belong to the stream (little-endian: low bytes first).
__device__ __forceinline__ uint32_t tail_mask(unsigned long long r, uint32_t w) {
  if (r >= 4ull * w + 4) return 0xFFFFFFFFu;
  if (r <= 4ull * w) return 0u;
  return (1u << (8u * (uint32_t)(r - 4ull * w))) - 1u;
}

// Granule k of a stream of l bytes at s (4-byte aligned; al: 16-byte aligned).
// Loads no word at or beyond align4(l); bytes at or beyond l come out zero.
__device__ __forceinline__ uint4 load_granule(const uint8_t* s, unsigned long long l, unsigned long long k, bool al) {
  const unsigned long long b = k << 4;
  const unsigned long long r = l - b;   // valid bytes from b on (> 0)
  uint4 v;
  if (al && r > 12) {   // the granule's last word starts inside the stream
    v = *reinterpret_cast<const uint4*>(s + b);
  } else {
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(s + b);
    v.x = sw[0];
    v.y = r > 4 ? sw[1] : 0u;
    v.z = r > 8 ? sw[2] : 0u;
    v.w = r > 12 ? sw[3] : 0u;
  }
  if (r < 16) {
    v.x &= tail_mask(r, 0);
    v.y &= tail_mask(r, 1);
    v.z &= tail_mask(r, 2);
    v.w &= tail_mask(r, 3);
  }
  return v;
}

// Ragged copy.  The off[n] / 16 destination granules are split evenly over the
// grid's waves (contiguous per block); a wave finds the stream that holds its
// first granule by binary search in off and walks the streams forward, one
// 16-byte granule per lane per step.  Everything but the lane's granule index
// is wave-uniform.  No granule that would end past cap is written.
__global__ __launch_bounds__(PK_COPY_THREADS) void pack_copy(const uint8_t* __restrict__ src, uint64_t stride,
                                                             const unsigned long long* __restrict__ len, uint32_t n,
                                                             const unsigned long long* __restrict__ off,
                                                             uint8_t* __restrict__ dst, unsigned long long cap) {
  const unsigned long long G = off[n] >> 4;
  const unsigned long long Gw = min(G, cap >> 4);   // granules that may be written
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wpb = PK_COPY_THREADS / 64;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned long long nw = (unsigned long long)gridDim.x * wpb;
  const unsigned long long wid = (unsigned long long)blockIdx.x * wpb + wave;
  const unsigned long long per = ((G + nw - 1) / nw + 63ull) & ~63ull;   // whole steps
  const unsigned long long g0 = wid * per;
  const unsigned long long g1 = min(g0 + per, Gw);
  if (g0 >= g1) return;
  // the last f with off[f] <= 16 * g0: off[0] = 0 and off[n] = 16 * G > 16 * g0,
  // and off[f + 1] > 16 * g0, so stream f is not empty and holds granule g0
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((off[mid] >> 4) <= g0) lo = mid;
    else hi = mid;
  }
  uint32_t f = lo;
  unsigned long long g = g0;
  uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst);
  while (g < g1) {   // (f < n: g < G = off[n] / 16)
    const unsigned long long fo = off[f] >> 4, fe = off[f + 1] >> 4;
    if (fe <= g) {   // an empty stream
      ++f;
      continue;
    }
    const unsigned long long l = min((unsigned long long)len[f], (fe - fo) << 4);
    const uint8_t* s = src + (uint64_t)f * stride;
    const bool al = (reinterpret_cast<uintptr_t>(s) & 15u) == 0;
    const unsigned long long kend = min(fe, g1) - fo;   // this wave's granules of f: [k, kend)
    unsigned long long k = g - fo;
    // whole granules (k < l / 16), PK_UNROLL per lane: every load issued before the stores
    const unsigned long long kfull = min(kend, l >> 4);
    if (al) {
      const uint4* s4 = reinterpret_cast<const uint4*>(s);
      for (; k + 64ull * PK_UNROLL <= kfull; k += 64ull * PK_UNROLL) {
        uint4 v[PK_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < PK_UNROLL; ++u) v[u] = s4[k + 64u * u + lane];
#pragma unroll
        for (uint32_t u = 0; u < PK_UNROLL; ++u) d4[fo + k + 64u * u + lane] = v[u];
      }
    } else {
      const uint32_t* sw = reinterpret_cast<const uint32_t*>(s);
      for (; k + 64ull * PK_UNROLL <= kfull; k += 64ull * PK_UNROLL) {
        uint4 v[PK_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < PK_UNROLL; ++u) {
          const uint32_t* q = sw + 4ull * (k + 64u * u + lane);
          v[u] = make_uint4(q[0], q[1], q[2], q[3]);
        }
#pragma unroll
        for (uint32_t u = 0; u < PK_UNROLL; ++u) d4[fo + k + 64u * u + lane] = v[u];
      }
    }
    // the rest, the stream's masked last granule included
    for (; k < kend; k += 64) {
      const unsigned long long kk = k + lane;
      if (kk < kend && (kk << 4) < l) d4[fo + kk] = load_granule(s, l, kk, al);
    }
    g = fo + kend;
    ++f;
  }
}

int pack_offsets_launch(void* stream, uint64_t stream_stride, const uint64_t* d_stream_len, uint32_t n_frames,
                        uint64_t packed_cap, uint64_t* d_off, int32_t* d_status) {
  hipLaunchKernelGGL(pack_scan, dim3(1), dim3(PK_SCAN_THREADS), 0, (hipStream_t)stream,
                     (const unsigned long long*)d_stream_len, stream_stride, n_frames, (unsigned long long*)d_off,
                     (unsigned long long)packed_cap, d_status);
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

int pack_streams_launch(void* stream, int cus, const uint8_t* d_streams, uint64_t stream_stride,
                        const uint64_t* d_stream_len, uint32_t n_frames, uint8_t* d_packed, uint64_t packed_cap,
                        uint64_t* d_off, int32_t* d_status) {
  hipStream_t st = (hipStream_t)stream;
  if (pack_offsets_launch(stream, stream_stride, d_stream_len, n_frames, packed_cap, d_off, d_status) != NICE_OK)
    return NICE_E_HIP;
  if (n_frames && packed_cap >= 16) {
    const uint32_t blocks = (uint32_t)std::max(cus, 1) * PK_COPY_BLOCKS_PER_CU;
    hipLaunchKernelGGL(pack_copy, dim3(blocks), dim3(PK_COPY_THREADS), 0, st, d_streams, stream_stride,
                       (const unsigned long long*)d_stream_len, n_frames, (const unsigned long long*)d_off, d_packed,
                       (unsigned long long)packed_cap);
  }
  return hipGetLastError() == hipSuccess ? NICE_OK : NICE_E_HIP;
}

}  // namespace nice
