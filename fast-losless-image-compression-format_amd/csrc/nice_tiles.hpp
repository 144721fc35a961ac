// nice_tiles.hpp -- what the byte-moving kernels of nice_tiles.hip (one tiled
// image) and nice_sets.hip (image sets) share: the block and unroll constants,
// the three move modes, the pixel loads and stores, and the band geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace nice {

constexpr uint32_t TL_THREADS = 256;
constexpr uint32_t TL_WAVES = TL_THREADS / 64;
constexpr uint32_t TL_UNROLL = 4;            // 4 x 1 KiB of loads in flight per wave on the 16-byte path
constexpr uint32_t TL_BLOCK_BYTES = 32768;   // a block's band of tile rows: about this many bytes

// how a row is moved: per pixel byte by byte (any channels, any alignment),
// per RGBA pixel as one dword, or four RGBA pixels as 16 bytes
enum TileMode { TL_BYTES = 0, TL_DWORD = 1, TL_QUAD = 2 };

__device__ __forceinline__ uint32_t tl_wave() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }

// One pixel of `c` (3 or 4) bytes at p, byte loads: bytes +0..+2 in the low 24
// bits, byte +3 (c == 4) or `fill` on top.
__device__ __forceinline__ uint32_t ld_px_bytes(const uint8_t* p, uint32_t c, uint32_t fill) {
  const uint32_t b0 = p[0], b1 = p[1], b2 = p[2];
  const uint32_t b3 = c == 4 ? (uint32_t)p[3] : fill;
  return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}
__device__ __forceinline__ void st_px_bytes(uint8_t* p, uint32_t c, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
  p[2] = (uint8_t)(v >> 16);
  if (c == 4) p[3] = (uint8_t)(v >> 24);
}

// Blocks per tile and tile rows per block for rows of row_bytes; false if
// slots * bands blocks do not fit a launch grid.
inline bool tl_bands(uint32_t slots, uint32_t th, uint64_t row_bytes, uint32_t& bands, uint32_t& rows_pb) {
  uint64_t rows = TL_BLOCK_BYTES / std::max<uint64_t>(row_bytes, 1);
  rows = std::min<uint64_t>(std::max<uint64_t>(rows, TL_WAVES), th);
  rows_pb = (uint32_t)rows;
  bands = (th + rows_pb - 1) / rows_pb;
  return (uint64_t)slots * bands <= 0x7FFFFFFFull;
}
inline bool tl_aligned(const void* p, uint64_t s, uint32_t a) { return ((uintptr_t)p & (a - 1)) == 0 && (s & (a - 1)) == 0; }

}  // namespace nice
