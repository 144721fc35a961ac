// nice_encode.hip -- MI355X (gfx950) encoder for the NICE2 bitstream.
//
// Pipeline per batch of same-shape frames (all kernels take the whole batch):
//   enc_classify   (nice_classify.hip) tiles of ENC_TILE consecutive pixels in
//                  raster order: per-pixel mode decision (code.rs:159-369),
//                  per-frame symbol histogram (hfe.rs:29-45), per-tile
//                  first/last coded pixel.
//   enc_tailruns   one block per frame: the run of each tile's last coded pixel
//                  may cross tiles; resolve it with a suffix-min over tiles and
//                  add its base-8 digits (code.rs:371-407) to the histogram.
//   enc_tables     one wave per (frame, stream): code lengths by exact replay of
//                  std BinaryHeap (hfe.rs:58-87), canonical codes (hfe.rs:255-296).
//   enc_header     one block per frame: file header (code.rs:72-84) + table
//                  header (hfe.rs:97-103) bits, data start position.
//   enc_pack       tiles again: per-pixel bit lengths, block scan, decoupled
//                  look-back across tiles for the bit offset (carrying the last
//                  32 bits so every output word is written once, no zero-fill,
//                  no global atomics), MSB-first packing (bitwriter.rs:55-73) and
//                  the tail (hfe.rs:115, code.rs:421-422).
//   enc_pack_long  frames whose emitted codes exceed FAST_MAX_CODE_BITS: the
//                  same tile-parallel placement with full-length codes, then
//                  the writes that wrap the reference's u32 cache (pending +
//                  length > 32, bitwriter.rs:63-64) applied to their 32-bit
//                  windows in a second pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nice_classify.hpp"
#include "nice_enc_shared.hpp"
#include "nice_format.h"
#include "nice_huffman.hpp"
#include "nice_kernels.h"
#include "nice_rec.hpp"

namespace nice {

// ---------------------------------------------------------------------------
// K2: runs crossing tile ends. One block (1024 threads) per frame.
// tile_next[t] = first coded pixel after tile t (N if none).
// ---------------------------------------------------------------------------
// Aggregate of each group of ENC_GROUP_TILES tiles (grid: groups x frames).
__global__ __launch_bounds__(GROUP_THREADS) void enc_group_reduce(EncArgs a, int what) {
  __shared__ unsigned long long part[4];
  const uint32_t g = blockIdx.x, f = blockIdx.y;
  if (what == 1 && !(a.frame_flags[f] & FLAG_LONG)) return;   // bit totals: long path only
  const uint32_t nt = a.tile_hi - a.tile_lo;
  const uint32_t t0 = g * ENC_GROUP_TILES, t1 = min(t0 + ENC_GROUP_TILES, nt);
  const uint64_t base = (uint64_t)f * a.tiles_per_frame + a.tile_lo;
  unsigned long long v = what == 0 ? NONE : 0ull;
  for (uint32_t t = t0 + threadIdx.x; t < t1; t += 256) {
    if (what == 0) v = min(v, (unsigned long long)a.tile_first[base + t]);
    else v += a.tile_bits[base + t];
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o);
    v = what == 0 ? min(v, w) : v + w;
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long r = part[0];
    for (int k = 1; k < 4; ++k) r = what == 0 ? min(r, part[k]) : r + part[k];
    a.gacc[(uint64_t)f * a.groups + g] = r;
  }
}

__global__ __launch_bounds__(TR_THREADS) void enc_tailruns(EncArgs a) {
  __shared__ uint32_t chunk_min[TR_THREADS];
  __shared__ uint32_t digits[8];   // run-digit counts, added to the histogram once
  if (threadIdx.x < 8) digits[threadIdx.x] = 0;
  // block (group g, frame f): tiles [g, g + 1) x ENC_GROUP_TILES of the band
  const uint32_t g = blockIdx.x, f = blockIdx.y;
  const uint32_t T = a.tiles_per_frame;
  const uint32_t ntb = a.tile_hi - a.tile_lo;
  const uint32_t g0 = g * ENC_GROUP_TILES;
  const uint64_t base = (uint64_t)f * T + a.tile_lo + g0;
  const uint32_t nt = min(ntb - g0, ENC_GROUP_TILES);
  const uint32_t N = a.W * a.H;
  // the first coded pixel after the group: later groups, then after the band
  // (frames: none)
  uint32_t after = a.band ? (a.band_next_dev ? *a.band_next_dev : (uint32_t)a.band_next) : NONE;
  for (uint32_t k = g + 1; k < a.groups; ++k) after = min(after, (uint32_t)a.gacc[(uint64_t)f * a.groups + k]);
  const uint32_t per = (nt + TR_THREADS - 1) / TR_THREADS;
  const uint32_t c0 = threadIdx.x * per;
  const uint32_t c1 = min(c0 + per, nt);
  uint32_t m = NONE;
#pragma unroll 8
  for (uint32_t t = c0; t < c1; ++t) m = min(m, a.tile_first[base + t]);
  chunk_min[threadIdx.x] = m;
  __syncthreads();
  // inclusive suffix-min over chunks (Hillis-Steele, 10 steps)
  for (int d = 1; d < TR_THREADS; d <<= 1) {
    uint32_t v = chunk_min[threadIdx.x];
    if (threadIdx.x + d < TR_THREADS) v = min(v, chunk_min[threadIdx.x + d]);
    __syncthreads();
    chunk_min[threadIdx.x] = v;
    __syncthreads();
  }
  uint32_t nxt = min((threadIdx.x + 1 < TR_THREADS) ? chunk_min[threadIdx.x + 1] : NONE, after);
#pragma unroll 8
  for (int64_t t = (int64_t)c1 - 1; t >= (int64_t)c0; --t) {
    const uint32_t next_px = (nxt == NONE) ? N : nxt;
    a.tile_next[base + t] = next_px;
    const uint32_t last = a.tile_last[base + t];
    if (last != NONE) {
      const uint64_t run = (uint64_t)next_px - last - 1;
      if (run > 0) {
        uint64_t mm = run - 1;
        while (true) {
          atomicAdd(&digits[mm & 7u], 1u);
          if (mm < 8) break;
          mm >>= 3;
        }
      }
    }
    nxt = min(nxt, a.tile_first[base + t]);
  }
  __syncthreads();
  if (threadIdx.x < 8 && digits[threadIdx.x])
    atomicAdd(&a.hist[(uint64_t)f * N_BINS + BIN_PREFIX + P_RUN1 + threadIdx.x], digits[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// K3: code lengths + canonical codes, one 64-lane wave per (frame, stream).
// table entry: code in bits [5, 31), length in bits [0, 5) when length <= 25;
// the full u8 length is also kept for the header (len8).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(ENC_WAVE_THREADS) void enc_tables(EncArgs a) {
  __shared__ HeapLds h;
  __shared__ uint32_t counts[MAX_ALPHABET];
  // stream-major, largest alphabets first (343, 256, 64, 64, 32 x 3, 13, 11,
  // 11 symbols): the long heap replays start in the first wave of blocks
  // instead of behind the short ones (a batch's blocks do not all fit at once)
  const uint32_t nf = gridDim.x / N_STREAMS;
  constexpr uint64_t ORDER = 5ull | 0ull << 4 | 2ull << 8 | 6ull << 12 | 3ull << 16 | 7ull << 20 | 8ull << 24 |
                             1ull << 28 | 4ull << 32 | 9ull << 36;
  const uint32_t f = blockIdx.x % nf;
  const int s = (int)((ORDER >> (4u * (blockIdx.x / nf))) & 15u);
  const int n = stream_size(s);
  const int sb = stream_base(s);
  const int lane = threadIdx.x;
  for (int i = lane; i < n; i += 64) counts[i] = a.hist[(uint64_t)f * N_BINS + sb + i];
  for (int i = lane; i < 2 * MAX_ALPHABET + 2; i += 64) h.parent[i] = -1;
  if (s == S_PREFIX) {   // the mode prefixes from their payload streams (every classify variant)
    __syncthreads();
    const uint32_t* hf = a.hist + (uint64_t)f * N_BINS;
    uint32_t c[5] = {0, 0, 0, 0, 0};
    for (int b = lane; b < N_BINS; b += 64) {
      const uint32_t v = hf[b];
#pragma unroll
      for (int k = 0; k < 5; ++k) c[k] += mode_id_bin(k, b) ? v : 0u;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      for (int o = 32; o > 0; o >>= 1) c[k] += (uint32_t)__shfl_xor((int)c[k], o);
      if (lane == k) counts[k] = c[k] / mode_id_syms(k);
    }
  }
  __syncthreads();
#ifdef NICE_PROF_TABLES
  const long long pt0 = clock64();
#endif
  huffman_merge_wave(h, counts, n);
  __syncthreads();
#ifdef NICE_PROF_TABLES
  const long long pt1 = clock64();
#endif
  // aob = 1 + number of merged ancestors (u8 wrapping, hfe.rs:79-82); the
  // lane's symbols' parent chains are walked together (independent loads)
  constexpr int SPL = (MAX_ALPHABET + 63) / 64;
  __shared__ uint32_t lvl_n[256], lvl_run[256];
  __shared__ unsigned long long lvl_cur[256];
  for (int b = lane; b < 256; b += 64) { lvl_n[b] = 0; lvl_run[b] = 0; }
  int pp[SPL];
  uint32_t ab[SPL];
#pragma unroll
  for (int q = 0; q < SPL; ++q) {
    const int i = lane + 64 * q;
    pp[q] = i < n ? h.parent[i] : -1;
    ab[q] = 1u;
  }
  while (true) {
    bool any = false;
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      if (pp[q] >= 0) {
        ++ab[q];
        pp[q] = h.parent[pp[q]];
        any = true;
      }
    }
    if (!__any(any)) break;
  }
  uint32_t my_max = 0, my_emit_max = 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < SPL; ++q) {
    const int i = lane + 64 * q;
    ab[q] &= 255u;
    if (i < n) {
      my_max = max(my_max, ab[q]);
      if (counts[i]) my_emit_max = max(my_emit_max, ab[q]);
      atomicAdd(&lvl_n[ab[q]], 1u);
    }
  }
  // canonical order (hfe.rs:264-270): lengths descending, then symbols
  // descending.  t = a symbol's place within its length = the symbols above it
  // with the same length: chunks of 64 from the top, one ballot per distinct
  // length in the chunk, running totals per length in LDS
  uint32_t t[SPL];
#pragma unroll
  for (int q = SPL - 1; q >= 0; --q) {
    const bool valid = lane + 64 * q < n;
    unsigned long long rem = __ballot(valid);
    t[q] = 0;
    while (rem) {
      const uint32_t av = (uint32_t)__builtin_amdgcn_readlane((int)ab[q], (int)__builtin_ctzll(rem));
      const bool mine = valid && ab[q] == av;
      const unsigned long long m = __ballot(mine);
      const uint32_t run = lvl_run[av];
      if (mine) t[q] = run + (uint32_t)__popcll(lane < 63 ? m >> (lane + 1) : 0ull);
      if (lane == 0) lvl_run[av] = run + (uint32_t)__popcll(m);
      rem &= ~m;
    }
  }
  // hfe.rs:271-290 (usize wrapping): the running code `cur` steps by one per
  // symbol within a length (not after a length-0 symbol: `prev > 0`) and is
  // shifted right by the length drop at each new length, so only its value at
  // each present length's first symbol is serial: one scalar pass over the
  // present lengths (ballots of the length histogram, bin a = lane a & 63 of
  // word a >> 6)
  __syncthreads();
  uint32_t ln_cnt[4];
  unsigned long long pres[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    ln_cnt[r] = lvl_n[64 * r + lane];
    pres[r] = __ballot(ln_cnt[r] != 0);
  }
  {
    unsigned long long cur = 0;
    uint32_t prev = 0;
    bool first = true;
#pragma unroll
    for (int r = 3; r >= 0; --r) {
      unsigned long long pm = pres[r];
      while (pm) {
        const uint32_t l = 63u - (uint32_t)__clzll(pm);
        pm &= ~(1ull << l);
        const uint32_t av = 64u * r + l;
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)ln_cnt[r], (int)l);
        if (!first) cur = (cur >> ((prev - av) & 63u)) + 1ull;   // prev > av >= 0: the shift, then prev > 0
        first = false;
        if (lane == 0) lvl_cur[av] = cur;
        cur += av ? (unsigned long long)(c - 1u) : 0ull;
        prev = av;
      }
    }
  }
  __syncthreads();
#ifdef NICE_PROF_TABLES
  const long long pt2 = clock64();
#endif
#pragma unroll
  for (int q = 0; q < SPL; ++q) {
    const int i = lane + 64 * q;
    if (i < n) {
      const uint32_t av = ab[q];
      const unsigned long long cur = lvl_cur[av] + (av ? t[q] : 0u);
      const unsigned long long code = (1ull << (av & 63u)) - cur - 1ull;
      const uint64_t e = (uint64_t)f * N_BINS + sb + i;
      a.tbl_len8[e] = (uint8_t)av;
      a.tbl_code[e] = (uint32_t)code;
    }
  }
  // wave max
  for (int o = 32; o > 0; o >>= 1) {
    my_max = max(my_max, (uint32_t)__shfl_xor((int)my_max, o));
    my_emit_max = max(my_emit_max, (uint32_t)__shfl_xor((int)my_emit_max, o));
  }
  if (lane == 0) {
    a.stream_max[(uint64_t)f * N_STREAMS + s] = (uint8_t)my_max;
#ifdef NICE_PROF_TABLES
    const long long pt3 = clock64();
    if (f == 0) printf("enc_tables stream %d n %d: merge %lld depth+rank %lld canon %lld cycles; wall %lld\n", s, n,
                       pt1 - pt0, pt2 - pt1, pt3 - pt2, (long long)wall_clock64());
#endif
    if (my_emit_max > FAST_MAX_CODE_BITS) {
      atomicOr(&a.frame_flags[f], FLAG_LONG);
      atomicOr(&a.frame_flags[a.n_frames], FLAG_LONG);   // any frame of the batch
    }
  }
}

// Test hook (nice_test_code_lengths): code lengths of n_vec count vectors of
// n symbols, one wave each, through the same heap replay as enc_tables.
__global__ __launch_bounds__(ENC_WAVE_THREADS) void enc_code_lengths_test(const uint32_t* counts, int n, uint8_t* aob) {
  __shared__ HeapLds h;
  __shared__ uint32_t c[MAX_ALPHABET];
  const uint32_t v = blockIdx.x;
  for (int i = threadIdx.x; i < n; i += 64) c[i] = counts[(uint64_t)v * n + i];
  for (int i = threadIdx.x; i < 2 * MAX_ALPHABET + 2; i += 64) h.parent[i] = -1;
  __syncthreads();
  huffman_merge_wave(h, c, n);
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 64) {
    uint32_t depth = 0;
    for (int p = h.parent[i]; p >= 0; p = h.parent[p]) ++depth;
    aob[(uint64_t)v * n + i] = (uint8_t)(1u + depth);
  }
}

// ---------------------------------------------------------------------------
// Exact replica of the reference Bitwriter (bitwriter.rs:17-73) for one lane,
// writing bytes to global memory.
// ---------------------------------------------------------------------------
struct DevBitwriter {
  uint8_t* out;
  uint64_t pos;   // bytes written
  uint8_t bit_offset;
  uint32_t cache;
  __device__ void write_8bits(uint8_t amount, uint8_t value) {
    bit_offset = (uint8_t)(bit_offset + amount);
    cache += ((uint32_t)value) << (((uint8_t)(32 - bit_offset)) & 31u);
    if (bit_offset >= 8) {
      out[pos++] = (uint8_t)(cache >> 24);
      bit_offset = (uint8_t)(bit_offset - 8);
      cache <<= 8;
    }
  }
  __device__ void write_24bits(uint8_t amount, uint32_t value) {
    bit_offset = (uint8_t)(bit_offset + amount);
    cache += value << (((uint8_t)(32 - bit_offset)) & 31u);
    while (bit_offset >= 8) {
      out[pos++] = (uint8_t)(cache >> 24);
      bit_offset = (uint8_t)(bit_offset - 8);
      cache <<= 8;
    }
  }
};

__device__ __forceinline__ uint8_t field_bits(uint8_t max_aob) {
  // u8::next_power_of_two().count_zeros() in release mode (hfe.rs:102)
  uint32_t np;
  if (max_aob <= 1) np = 1;
  else if (max_aob > 128) np = 0;
  else np = 1u << (32 - __builtin_clz((uint32_t)max_aob - 1u));
  return (uint8_t)(8 - __builtin_popcount(np));
}

// ---------------------------------------------------------------------------
// K4: headers. One wave per frame. Writes bytes [0, 4*floor(data_start/32)) and
// the frame's data start bit.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(ENC_WAVE_THREADS) void enc_header(EncArgs a) {
  __shared__ uint32_t words[200];   // 6160 bits = 192.5 words in the normal layout
  const uint32_t f = blockIdx.x;
  const int lane = threadIdx.x;
  uint8_t* out = a.out + (uint64_t)f * a.out_stride;
  const uint8_t* smax = a.stream_max + (uint64_t)f * N_STREAMS;
  bool normal = true;
  for (int s = 0; s < N_STREAMS; ++s) normal &= smax[s] <= 31;
  const uint64_t N = (uint64_t)a.W * a.H;

  if (normal && N > 0) {
    // Every field sits at a fixed bit offset: assemble 32-bit MSB-first words.
    for (int w = lane; w < 200; w += 64) words[w] = 0;
    __syncthreads();
    if (lane == 0) {
      words[0] = ('n' << 24) | ('i' << 16) | ('c' << 8) | 'e';
      words[1] = a.W;
      words[2] = a.H;
    }
    __syncthreads();
    if (lane == 0) atomicOr(&words[3], (uint32_t)a.channels_out << 24);
    // field list: for stream s: 5-bit max at bit pos, then n x 7-bit lengths
    uint32_t pos = 104;
    for (int s = 0; s < N_STREAMS; ++s) {
      const int n = stream_size(s);
      if (lane == 0) {
        const uint32_t v = smax[s], p = pos;
        const uint32_t w = p >> 5, o = p & 31;
        if (o + 5 <= 32) atomicOr(&words[w], v << (32 - o - 5));
        else { atomicOr(&words[w], v >> (o + 5 - 32)); atomicOr(&words[w + 1], v << (64 - o - 5)); }
      }
      pos += 5;
      for (int i = lane; i < n; i += 64) {
        const uint32_t v = a.tbl_len8[(uint64_t)f * N_BINS + stream_base(s) + i];
        const uint32_t p = pos + 7u * i;
        const uint32_t w = p >> 5, o = p & 31;
        if (o + 7 <= 32) atomicOr(&words[w], v << (32 - o - 7));
        else { atomicOr(&words[w], v >> (o + 7 - 32)); atomicOr(&words[w + 1], v << (64 - o - 7)); }
      }
      pos += 7u * n;
    }
    __syncthreads();
    // pos == 104 + 6056 = 6160; write words [0, 193): the last one partial,
    // zero past the header (the first data tile ORs into it)
    const uint32_t nwords = (pos + 31) >> 5;
    for (int w = lane; w < (int)nwords; w += 64)
      reinterpret_cast<uint32_t*>(out)[w] = __builtin_bswap32(words[w]);
    if (lane == 0) a.seed_bit[f] = pos;
    return;
  }
  if (lane != 0) return;
  // Serial exact path (spilled 5-bit fields, 8-bit fields, empty frames).
  for (int k = 0; k < 4; ++k) out[k] = "nice"[k];
  for (int k = 0; k < 4; ++k) out[4 + k] = (uint8_t)(a.W >> (24 - 8 * k));
  for (int k = 0; k < 4; ++k) out[8 + k] = (uint8_t)(a.H >> (24 - 8 * k));
  out[12] = a.channels_out;
  DevBitwriter bw{out, 13, 0, 0};
  for (int s = 0; s < N_STREAMS; ++s) {
    const uint8_t mx = smax[s];
    bw.write_8bits(5, mx);
    const uint8_t fb = field_bits(mx);
    for (int i = 0; i < stream_size(s); ++i)
      bw.write_8bits(fb, a.tbl_len8[(uint64_t)f * N_BINS + stream_base(s) + i]);
  }
  const uint64_t pos = bw.pos * 8 + bw.bit_offset;
  a.seed_bit[f] = pos;
  if (N > 0) {
    // pending bits (top bit_offset bits of the cache), then zeros to the end of
    // the word holding the data start: the first data tile ORs into it
    const uint64_t wend = ((pos >> 5) + 1) * 4;
    out[bw.pos] = bw.bit_offset ? (uint8_t)((bw.cache >> 24) & (0xFFu << (8 - bw.bit_offset))) : 0u;
    for (uint64_t q = bw.pos + 1; q < wend; ++q) out[q] = 0;
  }
  if (N == 0) {
    // no data symbols: tail only (hfe.rs:115, code.rs:421-422)
    const uint8_t P = (uint8_t)(bw.cache >> 24);
    uint64_t p = bw.pos;
    out[p++] = P;
    out[p++] = (uint8_t)(bw.cache >> 24);
    out[p++] = (uint8_t)(bw.cache >> 16);
    out[p++] = (uint8_t)(bw.cache >> 8);
    out[p++] = (uint8_t)(bw.cache);
    a.out_len[f] = p;
  }
}

// ---------------------------------------------------------------------------
// K5-K7: bit placement.
//   enc_packtab   per frame: the packer's code tables (nice_rec.hpp PackTab):
//                 each record slot -> {code, length}, T0 with the mode prefix
//                 composed in front, run digits composed per run length;
//                 FLAG_LONG for frames an entry of which exceeds 32 bits
//   enc_pack      per tile, one pass: the pixels' codes from three lookups
//                 each, a block scan of their lengths, the tile's stream
//                 offset by a decoupled look-back over the preceding tiles'
//                 status words (frames: from the data start; bands: from
//                 band_bit0), codes MSB-first into an LDS bit buffer
//                 (bitwriter.rs:55-73), then shifted to the offset and stored
//   enc_edges     ORs each group's first partial word into the word the group
//                 before it (or the header) wrote
//   enc_tail      per frame: [P, P, 0, 0, 0] after the data (hfe.rs:115,
//                 code.rs:421-422) and the stream length
// FLAG_LONG frames (a code over FAST_MAX_CODE_BITS, or a composed entry over
// 32 bits) take enc_tilebits -> enc_tilescan -> enc_pack_long instead.
// A thread owns 4 consecutive pixels and reads their records with one 16-byte
// load.
// ---------------------------------------------------------------------------
// LDS bit buffer: <= NICE_PACK_CAP_BPP bits per pixel on average over a group
// (denser groups go to enc_pack_over)
constexpr int PACK_CAP_BITS = PACK_SUB * ENC_TILE * NICE_PACK_CAP_BPP;
constexpr int PACK_MAX_WORDS = PACK_CAP_BITS / 32 + 2;

struct TileQuad {
  uint32_t rc[4];
  uint32_t nib;        // coded flags of the 4 pixels
};

// The thread's 4 records of tile tt of frame f (run members past the frame end).
__device__ __forceinline__ void quad_fetch(const EncArgs& a, uint32_t f, uint32_t tt, int p0, uint32_t (&rc)[4]) {
  const int64_t N = (int64_t)a.W * a.H;
  const int64_t start = (int64_t)tt * ENC_TILE;
  const int count = (int)((N - start) < ENC_TILE ? (N - start) : ENC_TILE);
  const uint32_t* rp = a.recs + (uint64_t)f * a.rec_stride + start + p0;
  if (p0 + 3 < count) {
    const uint4 v = *reinterpret_cast<const uint4*>(rp);
    rc[0] = v.x; rc[1] = v.y; rc[2] = v.z; rc[3] = v.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) rc[q] = (p0 + q < count) ? rp[q] : rec2_unc(0);
  }
}

// The tile's coded mask from the records (LDS, needs a barrier before use).
__device__ __forceinline__ void quad_mask(const uint32_t (&rc)[4], int lane, int wid, uint32_t* mask,
                                          TileQuad& Q) {
#pragma unroll
  for (int q = 0; q < 4; ++q) Q.rc[q] = rc[q];
  Q.nib = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) Q.nib |= (rec2_coded(Q.rc[q]) ? 1u : 0u) << q;
  const uint32_t mw = wave_or8(Q.nib << (4 * (lane & 7)));
  if ((lane & 7) == 0) mask[wid * 8 + (lane >> 3)] = mw;
}

// Run after each of the thread's 4 pixels (0 for run members): the next coded
// pixel in the thread's quad, else in the tile (mask), else tile_next.  Pixel
// indices are < 2^30 (the boundary's frame cap): 32-bit arithmetic.
__device__ __forceinline__ void quad_runs(const uint32_t* mask, int64_t start, int count, int p0,
                                          uint32_t next_tile_px, const TileQuad& Q, uint32_t (&run)[4]) {
  const int nx_local = next_coded_local(mask, p0 + 3);
  const uint32_t s32 = (uint32_t)start + (uint32_t)p0;
  const uint32_t after = (nx_local < count) ? (uint32_t)start + (uint32_t)nx_local : next_tile_px;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t later = Q.nib >> (q + 1);
    const uint32_t nxt = later ? s32 + (uint32_t)(q + 1) + (uint32_t)__builtin_ctz(later) : after;
    run[q] = ((Q.nib >> q) & 1u) ? nxt - (s32 + (uint32_t)q) - 1u : 0u;
  }
}

__device__ __forceinline__ void load_lens(uint32_t* lens, const EncArgs& a, uint32_t f) {
  for (int b = threadIdx.x; b < N_BINS; b += ENC_THREADS) lens[b] = a.tbl_len8[(uint64_t)f * N_BINS + b];
}

// Bits of the thread's 4 pixels (prefix, payload, run digits) from full code
// lengths (any length).
__device__ __forceinline__ uint32_t quad_nbits(const uint32_t* lens, const uint32_t* mask, int64_t start, int count,
                                               int p0, uint32_t next_tile_px, const TileQuad& Q) {
  uint32_t run[4];
  quad_runs(mask, start, count, p0, next_tile_px, Q, run);
  uint32_t nb = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t b[5];
    const uint32_t n = rec2_syms(Q.rc[q], b);
    for (uint32_t k = 0; k < n; ++k) nb += lens[b[k]];
    if (run[q] > 0) {
      uint32_t m = run[q] - 1;
      while (true) {
        nb += lens[BIN_PREFIX + P_RUN1 + (m & 7u)];
        if (m < 8) break;
        m >>= 3;
      }
    }
  }
  return nb;
}

// Contiguous tile ranges per block (the code table is reloaded only when the
// frame changes).  Work items w in [w0, w1): frame w / nt, band tile tile_lo + w % nt.
__device__ __forceinline__ void tile_range(const EncArgs& a, uint64_t& w0, uint64_t& w1) {
  const uint64_t total = (uint64_t)a.n_frames * (a.tile_hi - a.tile_lo);
  const uint64_t per = (total + gridDim.x - 1) / gridDim.x;
  w0 = (uint64_t)blockIdx.x * per;
  w1 = w0 + per < total ? w0 + per : total;
}

// frames (bands) the long-code path handles: those with FLAG_LONG
__device__ __forceinline__ bool long_path(const EncArgs& a, uint32_t f) {
  return (a.frame_flags[f] & FLAG_LONG) && !(a.frame_flags[f] & FLAG_BAD);
}

__global__ __launch_bounds__(ENC_THREADS) void enc_tilebits(EncArgs a) {
  __shared__ uint32_t tbl[N_BINS];
  __shared__ uint32_t mask[ENC_TILE / 32];
  __shared__ uint32_t wsum[ENC_THREADS / 64];
  if (!(a.frame_flags[a.n_frames] & FLAG_LONG)) return;   // no long-code frame in the batch
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t N = (int64_t)a.W * a.H;
  const int p0 = 4 * threadIdx.x;
  uint32_t cur_f = 0xFFFFFFFFu;
  uint64_t t0, t1;
  tile_range(a, t0, t1);
  TileIter it(a, t0);
  for (uint64_t w = t0; w < t1; ++w, it.step(1)) {
    const uint64_t t = it.tile();
    const uint32_t f = it.f, tt = it.tt();
    if (!long_path(a, f)) continue;   // block-uniform
    uint32_t rc[4];
    quad_fetch(a, f, tt, p0, rc);
    const int64_t start = (int64_t)tt * ENC_TILE;
    const int count = (int)((N - start) < ENC_TILE ? (N - start) : ENC_TILE);
    __syncthreads();
    if (f != cur_f) { load_lens(tbl, a, f); cur_f = f; }
    TileQuad Q;
    quad_mask(rc, lane, wid, mask, Q);
    __syncthreads();
    uint32_t x = quad_nbits(tbl, mask, start, count, p0, a.tile_next[t], Q);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    if (lane == 0) wsum[wid] = x;
    __syncthreads();
    if (threadIdx.x == 0) a.tile_bits[t] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  }
}

// One 1024-thread block per frame.
// block (group g, frame f): tiles [g, g + 1) x ENC_GROUP_TILES of the band,
// from the bits of the earlier groups on
__global__ __launch_bounds__(SCAN_THREADS) void enc_tilescan(EncArgs a) {
  __shared__ unsigned long long part[1024];
  const uint32_t g = blockIdx.x, f = blockIdx.y;
  if (!long_path(a, f)) return;
  const uint32_t g0 = g * ENC_GROUP_TILES;
  const uint32_t nt = min(a.tile_hi - a.tile_lo - g0, ENC_GROUP_TILES);
  const uint64_t base = (uint64_t)f * a.tiles_per_frame + a.tile_lo + g0;
  unsigned long long before = 0;
  for (uint32_t k = 0; k < g; ++k) before += a.gacc[(uint64_t)f * a.groups + k];
  const uint32_t per = (nt + 1023) / 1024;
  const uint32_t c0 = threadIdx.x * per, c1 = min(c0 + per, nt);
  unsigned long long sum = 0;
#pragma unroll 8
  for (uint32_t t = c0; t < c1; ++t) sum += a.tile_bits[base + t];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const unsigned long long v = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0ull;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  // frames: data starts after the header, whose last word is already zero
  // padded; bands: at band_bit0, and every partial word is shared (zeroed)
  const uint64_t seed = a.band ? a.band_bit0 : a.seed_bit[f];
  const int64_t seed_word = a.band ? (int64_t)(seed >> 5) - 1 : (int64_t)(seed >> 5);
  uint32_t* out32 = reinterpret_cast<uint32_t*>(a.out + (uint64_t)f * a.out_stride);
  unsigned long long run = seed + before + (threadIdx.x ? part[threadIdx.x - 1] : 0ull);
#pragma unroll 8
  for (uint32_t t = c0; t < c1; ++t) {
    a.tile_off[base + t] = run;
    // a word shared with the previous tile (or the header: pre-padded with zeros)
    if ((run & 31) && (int64_t)(run >> 5) > seed_word) out32[run >> 5] = 0u;
    run += a.tile_bits[base + t];
  }
  if (threadIdx.x == 1023 && g + 1 == a.groups) {
    const uint64_t end = seed + before + part[1023];
    a.data_end[f] = end;
    if ((end & 31) && (int64_t)(end >> 5) > seed_word) out32[end >> 5] = 0u;
  }
}

// The packer's tables of frame f (nice_rec.hpp).  An entry composes the codes
// of its symbols in emission order; entries whose symbols all occur in the
// frame must fit 32 bits with every code <= FAST_MAX_CODE_BITS, else the frame
// is FLAG_LONG (entries of absent symbols are never looked up).
__global__ __launch_bounds__(PACKTAB_THREADS) void enc_packtab(EncArgs a) {
  __shared__ uint32_t code[N_BINS];
  __shared__ uint8_t len[N_BINS], pres[N_BINS];
  __shared__ uint32_t s_long;
  const uint32_t f = blockIdx.x;
  if (a.frame_flags[f] & FLAG_LONG) return;
  const int tid = threadIdx.x;
  for (int b = tid; b < N_BINS; b += 256) {
    const uint64_t e = (uint64_t)f * N_BINS + b;
    code[b] = a.tbl_code[e];
    len[b] = a.tbl_len8[e];
    pres[b] = a.hist[e] != 0;
  }
  if (tid == 0) s_long = 0;
  __syncthreads();
  PackTab* out = reinterpret_cast<PackTab*>(a.packtab) + f;
  bool lng = false;
  // symbols b[k0 .. n) composed; presence from the payload symbols b[p0 .. n)
  auto ent = [&](const uint32_t* b, uint32_t k0, uint32_t n, uint32_t p0) -> uint2 {
    uint32_t L = 0, mx = 0;
    bool present = true;
    for (uint32_t k = k0; k < n; ++k) {
      L += len[b[k]];
      mx = max(mx, (uint32_t)len[b[k]]);
      if (k >= p0) present = present && pres[b[k]];
    }
    if (present && (L > 32u || mx > (uint32_t)FAST_MAX_CODE_BITS)) lng = true;
    if (L > 32u || mx > (uint32_t)FAST_MAX_CODE_BITS) return make_uint2(0u, 0u);
    uint64_t c = 0;
    for (uint32_t k = k0; k < n; ++k) c = (c << len[b[k]]) | code[b[k]];
    return make_uint2((uint32_t)c, L);
  };
  for (uint32_t e = tid; e < C0_N; e += 256) {
    uint32_t b[5];
    const uint32_t n = rec2_syms((e << 3) | rec2_abs(0), b);
    // T0: the prefix and c0's symbols (LUMA: k and g)
    out->t0[e] = n ? ent(b, 0, n == 5 ? 3u : 2u, 1) : make_uint2(0u, 0u);
  }
  for (uint32_t s = tid; s < SX_N; s += 256) {
    uint32_t b1 = 0, b2 = 0;
    const bool live = s < SX_ABS;
    if (s < SX_L2) { b1 = s; b2 = s; }
    else if (s < SX_LUMA) { b1 = BIN_LUMA2_R + (s - SX_L2); b2 = BIN_LUMA2_B + (s - SX_L2); }
    else { b1 = BIN_LUMA_OTHER + (s - SX_LUMA); b2 = b1; }
    out->t1[s] = live ? ent(&b1, 0, 1, 0) : make_uint2(0u, 0u);
    out->t2[s] = live ? ent(&b2, 0, 1, 0) : make_uint2(0u, 0u);
  }
  for (uint32_t m = tid; m < RC_N; m += 256) {
    uint32_t b[2];
    uint32_t n = 0;
    if (m < RC_TWO) {   // natural digits of m (code.rs:391-406)
      b[n++] = BIN_PREFIX + P_RUN1 + (m & 7u);
      if (m >= 8) b[n++] = BIN_PREFIX + P_RUN1 + (m >> 3);
    } else if (m < RC_NONE) {   // the first two digits of a run of >= 65
      b[n++] = BIN_PREFIX + P_RUN1 + ((m - RC_TWO) & 7u);
      b[n++] = BIN_PREFIX + P_RUN1 + ((m - RC_TWO) >> 3);
    }
    out->rc[m] = n ? ent(b, 0, n, 0) : make_uint2(0u, 0u);
  }
  if (lng) atomicOr(&s_long, 1u);
  __syncthreads();
  if (tid == 0 && s_long) {
    atomicOr(&a.frame_flags[f], FLAG_LONG);
    atomicOr(&a.frame_flags[a.n_frames], FLAG_LONG);
  }
}

// Tile status words of the decoupled look-back: the tile's bit
// count (ST_AGG) as soon as it is known, then its absolute end bit (ST_INCL).
constexpr unsigned long long ST_AGG = 1ull << 62, ST_INCL = 2ull << 62, ST_VAL = (1ull << 62) - 1;
__device__ __forceinline__ void st_store(unsigned long long* p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long st_load(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// One wave: publishes the tile's count, sums the counts of the tiles before
// it back to the nearest one whose end is known (or to the frame start,
// `base`), publishes its own end; returns the tile's start bit.  w: the tile's
// status index; k: the tiles before it in its frame.  Every tile waited on
// was claimed earlier by a running block, which never waits on a later one.
// agg_out: the count was published already (ST_AGG).
__device__ unsigned long long lookback(unsigned long long* st, uint32_t w, uint32_t k, unsigned long long base,
                                       uint32_t bits, int lane, bool agg_out = false) {
  if (k == 0) {
    if (lane == 0) st_store(&st[w], ST_INCL | (base + bits));
    return base;
  }
  if (lane == 0 && !agg_out) st_store(&st[w], ST_AGG | bits);
  unsigned long long excl = 0;
  uint32_t j = w - 1, rem = k;
  while (true) {
    const bool valid = (uint32_t)lane < rem;
    const unsigned long long v = valid ? st_load(&st[j - lane]) : 0ull;
    const uint32_t state = (uint32_t)(v >> 62);
    const unsigned long long inc = __ballot(valid && state == 2u);
    const unsigned long long notready = __ballot(valid && state == 0u);
    const int first = inc ? (int)__builtin_ctzll(inc) : 64;
    const unsigned long long need = first >= 63 ? ~0ull : ((2ull << first) - 1ull);
    if (notready & need) {
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    unsigned long long x = (valid && lane <= first) ? (v & ST_VAL) : 0ull;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    excl += x;
    if (inc) break;
    if (rem <= 64) { excl += base; break; }
    j -= 64;
    rem -= 64;
  }
  if (lane == 0) st_store(&st[w], ST_INCL | (excl + bits));
  return excl;
}

// Work distribution of enc_pack (wave 0 of a block; f = NONE: no work left).
// Per-frame tile counters: block b serves slot b % I (I = pack_slots <= 64):
// frames slot, slot + I, ..., each frame's tiles claimed in order, then any
// frame with tiles left (scanned 64 counters at a time).  A frame is worked
// by about G / I blocks at once, so a look-back rarely reaches past one
// 64-tile window; a tile is claimed only when its block is about to pack it
// (the next claim goes out once this tile's offset is published), so every
// tile a look-back waits on publishes its count within one tile's time.
// pre: the result of a claim on f already issued by the caller (NONE: none).
__device__ void pack_next(const EncArgs& a, uint32_t nt, uint32_t I, uint32_t slot, uint32_t& f, uint32_t& k,
                          uint32_t& seq, int lane, uint32_t pre = NONE) {
  const uint32_t F = a.n_frames;
  while (true) {
    if (f != NONE) {
      uint32_t kk = pre;
      if (pre == NONE) {
        if (lane == 0) kk = atomicAdd(&a.pack_ctr[f], 1u);
        kk = (uint32_t)__shfl((int)kk, 0);
      }
      pre = NONE;
      if (kk < nt) { k = kk; return; }
    }
    const uint32_t own = slot + seq * I;
    if (own < F) {
      ++seq;
      f = (a.frame_flags[own] & (FLAG_LONG | FLAG_BAD)) ? NONE : own;   // long frames: enc_pack_long
      continue;
    }
    f = NONE;
    for (uint32_t b0 = 0; b0 < F; b0 += 64) {
      const uint32_t g = b0 + (uint32_t)lane;
      const bool cand = g < F && !(a.frame_flags[g] & (FLAG_LONG | FLAG_BAD)) &&
                        __hip_atomic_load(&a.pack_ctr[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < nt;
      const unsigned long long m = __ballot(cand);
      if (m) { f = b0 + (uint32_t)__builtin_ctzll(m); break; }
    }
    if (f == NONE) return;
  }
}

// The thread's 4 pixels of one tile: each pixel's codes (T0, T1, T2, run
// digits) composed into one value when they fit 32 bits, their bit count, the
// run digits past a long run's first two, and the thread's total.
struct QuadCodes {
  uint32_t v[4], tot[4], xm[4], ri[4], nb, tmax;
};
__device__ __forceinline__ uint2 pt_entry(const PackTab& tab, uint32_t r, int i) {
  // 8-byte entries at the record's field offsets (nice_rec.hpp: bits 3..13,
  // 14..22, 23..31)
  const char* tb = reinterpret_cast<const char*>(&tab);
  return i == 0 ? *reinterpret_cast<const uint2*>(tb + offsetof(PackTab, t0) + (r & 0x3FF8u))
       : i == 1 ? *reinterpret_cast<const uint2*>(tb + offsetof(PackTab, t1) + ((r >> 11) & 0xFF8u))
                : *reinterpret_cast<const uint2*>(tb + offsetof(PackTab, t2) + ((r >> 20) & 0xFF8u));
}
__device__ __forceinline__ void quad_codes(const PackTab& tab, const uint32_t* mask, int64_t start, int count, int p0,
                                           uint32_t next_tile_px, const TileQuad& Q, QuadCodes& C) {
  uint32_t run[4];
  quad_runs(mask, start, count, p0, next_tile_px, Q, run);
  C.nb = 0;
  C.tmax = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t r = Q.rc[q];
    const uint2 e0 = pt_entry(tab, r, 0), e1 = pt_entry(tab, r, 1), e2 = pt_entry(tab, r, 2);
    const uint32_t m = run[q] - 1u;
    C.ri[q] = run[q] == 0 ? RC_NONE : m < 64u ? m : RC_TWO + (m & 63u);
    const uint2 e3 = tab.rc[C.ri[q]];
    C.xm[q] = run[q] > 64u ? m >> 6 : 0u;
    C.tot[q] = e0.y + e1.y + e2.y + e3.y;
    // composed value, exact when tot <= 32 (shifts stay below 32 then)
    uint32_t v = e0.x;
    v = (v << (e1.y & 31u)) | e1.x;
    v = (v << (e2.y & 31u)) | e2.x;
    v = (v << (e3.y & 31u)) | e3.x;
    C.v[q] = v;
    C.tmax = max(C.tmax, C.tot[q]);
    C.nb += C.tot[q];
  }
  if (C.xm[0] | C.xm[1] | C.xm[2] | C.xm[3]) {   // run digits past a long run's first two (runs of >= 65)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      for (uint32_t xr = C.xm[q]; xr;) {
        C.nb += tab.rc[xr & 7u].y;
        if (xr < 8) break;
        xr >>= 3;
      }
    }
  }
}
// Every code of the thread's pixels, in order, through put(val, n) (n <= 32
// bits of val, 0 when n == 0): one put per pixel when every pixel of the wave
// fits 32 bits (the common case), else two (the entries read again), else one
// per entry.
template <class Put>
__device__ __forceinline__ void quad_emit(const PackTab& tab, const TileQuad& Q, const QuadCodes& C, Put&& put) {
  auto put_extra = [&](uint32_t xr) {
    while (true) {
      const uint2 d = tab.rc[xr & 7u];
      put(d.x, d.y);
      if (xr < 8) break;
      xr >>= 3;
    }
  };
  if (__all(C.tmax <= 32u)) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      put(C.v[q], C.tot[q]);
      if (C.xm[q]) put_extra(C.xm[q]);
    }
  } else if (__all(C.tmax <= 64u)) {
    for (int q = 0; q < 4; ++q) {
      const uint2 e0 = pt_entry(tab, Q.rc[q], 0), e1 = pt_entry(tab, Q.rc[q], 1), e2 = pt_entry(tab, Q.rc[q], 2);
      const uint2 e3 = tab.rc[C.ri[q]];
      uint64_t v = e0.x;
      v = (v << e1.y) | e1.x;
      v = (v << e2.y) | e2.x;
      v = (v << e3.y) | e3.x;
      const bool two = C.tot[q] > 32u;
      put(two ? (uint32_t)(v >> 32) : 0u, two ? C.tot[q] - 32u : 0u);
      put((uint32_t)v, two ? 32u : C.tot[q]);
      if (C.xm[q]) put_extra(C.xm[q]);
    }
  } else {
    for (int q = 0; q < 4; ++q) {
      for (int i = 0; i < 3; ++i) {
        const uint2 e = pt_entry(tab, Q.rc[q], i);
        put(e.x, e.y);
      }
      const uint2 e3 = tab.rc[C.ri[q]];
      put(e3.x, e3.y);
      if (C.xm[q]) put_extra(C.xm[q]);
    }
  }
}

// One work item of enc_pack is PACK_SUB consecutive tiles of a frame (a
// "group"): one claim and one look-back per 4096 pixels.  Wave k of the block
// packs tile k of the group: lane L owns pixels 16L .. 16L + 15 of the tile
// (four 16-byte record loads), composes each pixel's codes into one value of
// <= 32 bits (T0, T1, T2, the first two run digits; a pixel with longer codes
// puts its entries one by one), and a wave prefix sum of the lanes' bit
// counts gives each lane's bit position in its tile.  The group's tile totals
// (one block barrier) place the tiles in the group's LDS bit buffer; each
// lane streams its pieces MSB-first through a 64-bit register window and ORs
// each completed word into the buffer once: about 6 LDS atomics per 16 pixels
// (round 3's per-4-pixel puts made two per pixel, and spent 45 % of the LDS
// cycles in bank conflicts) and two block barriers per group instead of three
// per tile.  A group of over pack_cap_bits bits (over 32 per pixel on average)
// is counted first and then OR-ed into the output directly, tile by tile.
constexpr int PW_PX = ENC_TILE / 64;   // pixels per lane: 16

struct LanePx {
  uint32_t v[PW_PX];     // composed codes (exact where the pixel's length <= 32)
  uint32_t tot4[PW_PX / 4];   // lengths (<= 128: 8 bits each, four per word)
  const uint32_t* rp;    // the lane's records (re-read for pixels over 32 bits)
  uint32_t cm;           // coded flags of the lane's pixels
  uint32_t after;        // first coded pixel after the lane (absolute)
  uint32_t s;            // the lane's first pixel (absolute)
  uint32_t nb, tmax, rmax;   // bits, longest pixel, longest run after a pixel
  __device__ __forceinline__ uint32_t tot(int q) const { return (tot4[q >> 2] >> (8 * (q & 3))) & 0xFFu; }
};

// run after pixel q of the lane (0 for run members)
__device__ __forceinline__ uint32_t lane_run(const LanePx& P, int q) {
  const uint32_t later = P.cm >> (q + 1);
  const uint32_t nxt = later ? P.s + (uint32_t)(q + 1) + (uint32_t)__builtin_ctz(later) : P.after;
  return ((P.cm >> q) & 1u) ? nxt - (P.s + (uint32_t)q) - 1u : 0u;
}
__device__ __forceinline__ uint32_t rc_index(uint32_t run) {
  const uint32_t m = run - 1u;
  return run == 0 ? RC_NONE : m < 64u ? m : RC_TWO + (m & 63u);
}

// The lane's 16 pixels of tile tt of frame f: each pixel's composed code and
// length, the lane's bit count.  Pixel indices are < 2^30 (the boundary's
// frame cap): 32-bit arithmetic.
// The lane's 16 records of tile tt of frame f (issued early: enc_pack loads the
// next group's records while it places the current one).
__device__ __forceinline__ void lane_recs(const EncArgs& a, uint32_t f, uint32_t tt, int lane, uint32_t (&rec)[PW_PX]) {
  const int64_t N = (int64_t)a.W * a.H;
  const int64_t start = (int64_t)tt * ENC_TILE;
  const int count = (int)((N - start) < ENC_TILE ? (N - start) : ENC_TILE);
  const int p0 = PW_PX * lane;
  const uint32_t* rp = a.recs + (uint64_t)f * a.rec_stride + start + p0;
  if (p0 + PW_PX <= count) {
#pragma unroll
    for (int q = 0; q < PW_PX / 4; ++q) {
      const uint4 r = reinterpret_cast<const uint4*>(rp)[q];
      rec[4 * q] = r.x; rec[4 * q + 1] = r.y; rec[4 * q + 2] = r.z; rec[4 * q + 3] = r.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < PW_PX; ++q) rec[q] = (p0 + q < count) ? rp[q] : rec2_unc(0);
  }
}
// cmw: the tile's coded-flag words in the standard order (enc_rundigits wrote
// them; 16 bits per lane) when the frame's classify produced them, else null
// (bands, the window kernels): then the flags come from the records.
__device__ __forceinline__ void lane_codes(const EncArgs& a, const PackTab& tab, uint32_t f, uint32_t tt,
                                           uint32_t next_tile_px, int lane, const uint32_t (&rec)[PW_PX], LanePx& P,
                                           const uint32_t* cmw) {
  const int64_t start = (int64_t)tt * ENC_TILE;
  const int p0 = PW_PX * lane;
  P.rp = a.recs + (uint64_t)f * a.rec_stride + start + p0;
  if (cmw) {   // one load instead of an extract, compare and insert per pixel
    P.cm = (cmw[lane >> 1] >> (16u * ((uint32_t)lane & 1u))) & 0xFFFFu;
  } else {
    P.cm = 0;
#pragma unroll
    for (int q = 0; q < PW_PX; ++q) P.cm |= (rec2_coded(rec[q]) ? 1u : 0u) << q;
  }
  // the first coded pixel after the lane: in the next lane with one, else after the tile
  const unsigned long long lanes = __ballot(P.cm != 0u);
  const unsigned long long later = lane < 63 ? lanes >> (lane + 1) : 0ull;
  const int nl = later ? lane + 1 + (int)__builtin_ctzll(later) : 64;
  const uint32_t first_local = P.cm ? (uint32_t)p0 + (uint32_t)__builtin_ctz(P.cm) : 0u;
  const uint32_t nf = (uint32_t)__shfl((int)first_local, nl & 63);
  P.s = (uint32_t)start + (uint32_t)p0;
  P.after = nl < 64 ? (uint32_t)start + nf : next_tile_px;
  P.nb = 0;
  P.tmax = 0;
  P.rmax = 0;
  // each pixel's run-code index, from the last pixel back: the next coded
  // pixel is carried in a register instead of a bit scan per pixel
  uint32_t rci[PW_PX];
  {
    uint32_t nx = P.after - P.s;   // lane-relative
#pragma unroll
    for (int q = PW_PX - 1; q >= 0; --q) {
      const uint32_t cqm = (uint32_t)__builtin_amdgcn_sbfe((int)P.cm, q, 1);   // coded: ~0
      const uint32_t run = (nx - (uint32_t)q - 1u) & cqm;
      rci[q] = rc_index(run);
      P.rmax = max(P.rmax, run);   // (a per-pixel flag bit cost three VALU)
      // one bit insert (the compiler turned the and-or form into a shift,
      // compare, select and and-or)
      asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(nx) : "v"(cqm), "I"(q), "v"(nx));
    }
  }
#pragma unroll
  for (int q = 0; q < PW_PX; ++q) {
    if ((q & 3) == 0) {
      P.tot4[q >> 2] = 0;
      __builtin_amdgcn_sched_barrier(0);   // four pixels' lookups in flight at a time (registers)
    }
    const uint32_t r = rec[q];
    const uint2 e0 = pt_entry(tab, r, 0), e1 = pt_entry(tab, r, 1), e2 = pt_entry(tab, r, 2);
    const uint2 e3 = tab.rc[rci[q]];
    const uint32_t t = e0.y + e1.y + e2.y + e3.y;
    uint32_t v = e0.x;   // exact when t <= 32 (shifts stay below 32 then)
    v = (v << (e1.y & 31u)) | e1.x;
    v = (v << (e2.y & 31u)) | e2.x;
    v = (v << (e3.y & 31u)) | e3.x;
    asm volatile("" : "+v"(v) : "v"(t));   // materialise the pixel's code now (no entries kept live)
    P.v[q] = v;
    P.tot4[q >> 2] |= t << (8 * (q & 3));
    P.tmax = max(P.tmax, t);
    P.nb += t;
  }
  if (P.rmax > 64u) {   // run digits past a long run's first two (runs of >= 65)
    for (int q = 0; q < PW_PX; ++q) {
      const uint32_t run = lane_run(P, q);
      if (run <= 64u) continue;
      for (uint32_t xr = (run - 1u) >> 6; xr;) {
        P.nb += tab.rc[xr & 7u].y;
        if (xr < 8) break;
        xr >>= 3;
      }
    }
  }
}

// The lane's codes MSB-first from bit `pos` of the group's LDS buffer
// (bitwriter.rs:55-73 placement): a 64-bit window of pending bits, each
// completed word OR-ed in once (the first and last are shared with the
// neighbouring lanes; the buffer is zero).
__device__ __forceinline__ void lane_emit(const PackTab& tab, const LanePx& P, uint32_t* bits, uint32_t pos) {
  unsigned long long acc = 0;
  uint32_t n = pos & 31u;
  uint32_t* wp = bits + (pos >> 5);
  auto put = [&](uint32_t val, uint32_t len) {   // len <= 32, val < 2^len
    acc = (acc << len) | val;
    n += len;
    if (n >= 32u) {
      // the completed word, acc >> (n - 32), as one funnel shift (32 <= n < 64);
      // the word pointer steps instead of an index scaled per flush
      atomicOr(wp, __builtin_amdgcn_alignbit((uint32_t)(acc >> 32), (uint32_t)acc, n));
      ++wp;
      n -= 32u;
    }
  };
  if (__all(P.tmax <= 32u && P.rmax <= 64u)) {
    // every pixel of the wave one composed value, no run past 64 pixels
#pragma unroll
    for (int q = 0; q < PW_PX; ++q) put(P.v[q], P.tot(q));
  } else {
    // entry by entry from the records again (each entry <= 32 bits: longer
    // ones make the frame FLAG_LONG), then a long run's further digits
    for (int q = 0; q < PW_PX; ++q) {
      if ((P.cm >> q) & 1u) {   // coded (P.cm has no bits past the frame's end)
        const uint32_t r = P.rp[q], run = lane_run(P, q);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const uint2 e = pt_entry(tab, r, i);
          put(e.x, e.y);
        }
        const uint2 e3 = tab.rc[rc_index(run)];
        put(e3.x, e3.y);
        if (run > 64u) {
          for (uint32_t xr = (run - 1u) >> 6;;) {
            const uint2 d = tab.rc[xr & 7u];
            put(d.x, d.y);
            if (xr < 8) break;
            xr >>= 3;
          }
        }
      }
    }
  }
  if (n) atomicOr(wp, (uint32_t)(acc << (32u - n)));
}

__global__ __launch_bounds__(PK_THREADS, PACK_BLOCKS_PER_CU) void enc_pack(EncArgs a) {
  __shared__ PackTab tab;
  __shared__ uint32_t bits[PACK_MAX_WORDS];
  __shared__ uint32_t wsum[PK_THREADS / 64];
  __shared__ uint32_t s_f, s_k;
  __shared__ unsigned long long s_off;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t nt = a.tile_hi - a.tile_lo;
  const uint32_t ng = (nt + PACK_SUB - 1) / PACK_SUB;   // groups per frame
  const uint32_t T = a.tiles_per_frame;
  const uint32_t I = a.pack_slots, slot = blockIdx.x % a.pack_slots;
  uint32_t cf = NONE, ck = 0, seq = 0;   // wave 0's work cursor
#ifdef NICE_PACK_PROF
  long long pr[7] = {0, 0, 0, 0, 0, 0, 0}, pt = clock64(), pn = 0;
#define PROF_MARK(i) do { const long long c_ = clock64(); pr[i] += c_ - pt; pt = c_; } while (0)
#else
#define PROF_MARK(i) do {} while (0)
#endif
  if (wid == 0) {
    pack_next(a, ng, I, slot, cf, ck, seq, lane);
    if (lane == 0) { s_f = cf; s_k = ck; }
  }
  __syncthreads();
  uint32_t f = s_f, g = s_k;
  uint32_t cur_f = NONE, used_words = PACK_MAX_WORDS;
  uint32_t rec[PW_PX];    // the wave's tile records
  while (f != NONE) {
    const uint32_t k0 = g * PACK_SUB, nsub = min((uint32_t)PACK_SUB, nt - k0);
    const uint32_t tt0 = a.tile_lo + k0;
    const uint64_t t0 = (uint64_t)f * T + tt0;   // the group's first tile
    if (f != cur_f) {
      const uint4* src = reinterpret_cast<const uint4*>(a.packtab + (uint64_t)f * sizeof(PackTab));
      uint4* dst = reinterpret_cast<uint4*>(&tab);
      for (int i = tid; i < (int)(sizeof(PackTab) / 16); i += PK_THREADS) dst[i] = src[i];
      cur_f = f;
    }
    for (uint32_t i = tid; i < used_words; i += PK_THREADS) bits[i] = 0;
    __syncthreads();   // the frame's tables in LDS, the buffer clear
    PROF_MARK(0);
    // wave wid: tile tt0 + wid of the group
    LanePx P;
    uint32_t x = 0;
    const bool mine = (uint32_t)wid < nsub;   // wave-uniform
    if (mine) {
      lane_recs(a, f, tt0 + wid, lane, rec);
      lane_codes(a, tab, f, tt0 + wid, a.tile_next[(uint64_t)f * T + tt0 + wid], lane, rec, P,
                 a.cmask_std ? a.cmask + ((uint64_t)f * T + tt0 + wid) * (ENC_TILE / 32) : nullptr);
      x = wave_incl_scan(P.nb);
    }
    if (lane == 63) wsum[wid] = mine ? x : 0u;
    __syncthreads();
    uint32_t wbase = 0, gbits = 0;   // bits before this wave's tile, the group's bits
#pragma unroll
    for (int i = 0; i < PK_THREADS / 64; ++i) {
      const uint32_t ws = wsum[i];
      wbase += (i < wid) ? ws : 0u;
      gbits += ws;
    }
    // (waves ranked by their bits at priorities 3..0 for the puts: no
    // faster, r06zv_ab_pack_place.log)
    PROF_MARK(1);
    const bool over = gbits > a.pack_cap_bits;   // block-uniform
#ifndef NICE_PACK_LATE_AGG
    // the group's count goes out before the puts: the look-backs of the
    // groups after it wait on it (a look-back was ~40 % of a group's time)
    const bool agg_out = g > 0;
    if (agg_out && tid == 0) st_store(&a.status[f * ng + g], ST_AGG | gbits);
#else
    const bool agg_out = false;
#endif
    if (!over && mine && P.nb) lane_emit(tab, P, bits, wbase + x - P.nb);
    PROF_MARK(2);
    if (wid == 0) {
      // the look-back first: the groups behind wait on its published prefix
      // (pack 8.12 -> 8.04 ms per 512 frames, profiles/r06zg_ab_prio.log)
      __builtin_amdgcn_s_setprio(3);
      const unsigned long long off = lookback(a.status, f * ng + g, g, a.band ? a.band_bit0 : a.seed_bit[f], gbits, lane,
                                              agg_out);
      if (lane == 0) s_off = off;
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
    PROF_MARK(3);
    // place the group's bits at its stream offset
    const unsigned long long s0 = s_off, e0 = s0 + gbits;
    const uint32_t sh = (uint32_t)(s0 & 31);
    const uint64_t w0 = s0 >> 5;
    const uint32_t nw = gbits ? (uint32_t)(((e0 + 31) >> 5) - w0) : 0u;
    uint32_t* out32 = reinterpret_cast<uint32_t*>(a.out + (uint64_t)f * a.out_stride);
    if (!over) {
      for (uint32_t m = tid; m < nw; m += PK_THREADS) {
        const uint32_t hi = m ? bits[m - 1] : 0u;
        const uint32_t lo = bits[m];   // zero past the group's bits
        const uint32_t v = sh ? (uint32_t)((((uint64_t)hi << 32) | lo) >> sh) : lo;
        // a word is stored by the group holding its first bit (zeros past
        // the group's end); this group's bits in the word holding its
        // start go to enc_edges
        if (m == 0 && sh) a.tile_bits[t0] = v;
        else out32[w0 + m] = __builtin_bswap32(v);
      }
    } else if (tid == 0) {
      // over the LDS buffer: listed for enc_pack_over (after this kernel, before enc_edges)
      const uint32_t k = atomicAdd(a.over_count, 1u);
      a.over_list[k] = make_uint2(f * ng + g, gbits);
    }
    if (tid == 0) {
      a.tile_off[t0] = s0;
      if (over || !(nw && sh)) a.tile_bits[t0] = 0u;
      if (tt0 + nsub == T) a.data_end[f] = e0;
    }
    used_words = over ? 0u : nw + 1;   // an over-cap group writes nothing into the buffer
    PROF_MARK(4);
    // the next group: claimed only now, when this block can start it at once
    // (a group claimed earlier would keep the look-backs of the groups after
    // it waiting while its block finishes this one; claiming during the
    // placement, or loading the next group's records then, measured no
    // faster: r04e, r04n)
    if (wid == 0) {
      __builtin_amdgcn_s_setprio(3);   // (the block waits on the claim: pack 7.96 -> 7.90 ms, r06zo)
      pack_next(a, ng, I, slot, cf, ck, seq, lane);
      __builtin_amdgcn_s_setprio(0);
      if (lane == 0) { s_f = cf; s_k = ck; }
    }
    __syncthreads();
    f = s_f;
    g = s_k;
    PROF_MARK(5);
#ifdef NICE_PACK_PROF
    ++pn;
#endif
  }
#ifdef NICE_PACK_PROF
  if (tid == 0 && (blockIdx.x % 256) == 0)
    printf("enc_pack block %u: groups %lld cycles/group: wait+mask %lld codes+scan %lld puts %lld lookback %lld "
           "place %lld claim %lld\n", blockIdx.x, pn, pr[0] / max(pn, 1ll), pr[1] / max(pn, 1ll),
           pr[2] / max(pn, 1ll), pr[3] / max(pn, 1ll), pr[4] / max(pn, 1ll), pr[5] / max(pn, 1ll));
#endif
}

// Groups over enc_pack's LDS buffer (pack_cap_bits: over 32 bits per pixel on
// average), listed by enc_pack with their bit counts, once every group's
// offset is published: the words whose first bit is the group's are zeroed,
// then each code is OR-ed into place tile by tile (the word holding the
// group's first bit through tile_bits, for enc_edges).  Rare; kept out of
// enc_pack, whose registers it would otherwise take.
__global__ __launch_bounds__(PK_THREADS) void enc_pack_over(EncArgs a) {
  __shared__ PackTab tab;
  __shared__ uint32_t mask[ENC_TILE / 32];
  __shared__ uint32_t wsum[PK_THREADS / 64];
  const uint32_t n_over = *a.over_count;
  if (blockIdx.x >= n_over) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t nt = a.tile_hi - a.tile_lo;
  const uint32_t ng = (nt + PACK_SUB - 1) / PACK_SUB;
  const uint32_t T = a.tiles_per_frame;
  const int64_t N = (int64_t)a.W * a.H;
  const int p0 = 4 * tid;
  uint32_t rc[4];
  for (uint32_t item = blockIdx.x; item < n_over; item += gridDim.x) {
    const uint2 it = a.over_list[item];
    const uint32_t f = it.x / ng, g = it.x % ng, gbits = it.y;
    const uint32_t k0 = g * PACK_SUB, nsub = min((uint32_t)PACK_SUB, nt - k0);
    const uint32_t tt0 = a.tile_lo + k0;
    const uint64_t t0 = (uint64_t)f * T + tt0;
    __syncthreads();   // the previous item's readers of tab
    {
      const uint4* src = reinterpret_cast<const uint4*>(a.packtab + (uint64_t)f * sizeof(PackTab));
      uint4* dst = reinterpret_cast<uint4*>(&tab);
      for (int i = tid; i < (int)(sizeof(PackTab) / 16); i += PK_THREADS) dst[i] = src[i];
    }
    const unsigned long long s0 = a.tile_off[t0], e0 = s0 + gbits;
    const uint32_t sh = (uint32_t)(s0 & 31);
    const uint64_t w0 = s0 >> 5;
    uint32_t* out32 = reinterpret_cast<uint32_t*>(a.out + (uint64_t)f * a.out_stride);
      // zero the words only this group writes (every word whose first bit is
      // the group's), then OR each code into place, tile by tile
      const uint64_t z0 = (s0 + 31) >> 5, z1 = (e0 + 31) >> 5;
      for (uint64_t m = z0 + tid; m < z1; m += PK_THREADS) out32[m] = 0u;
      if (tid == 0) a.tile_bits[t0] = 0u;
      __threadfence();
      __syncthreads();
      auto or_word = [&](uint64_t wd, uint32_t v) {
        if (!v) return;
        if (sh && wd == w0) atomicOr(&a.tile_bits[t0], v);
        else atomicOr(&out32[wd], __builtin_bswap32(v));
      };
      unsigned long long run = s0;
      for (uint32_t s = 0; s < nsub; ++s) {
        const uint32_t tt = tt0 + s;
        const int64_t start = (int64_t)tt * ENC_TILE;
        const int count = (int)((N - start) < ENC_TILE ? (N - start) : ENC_TILE);
        quad_fetch(a, f, tt, p0, rc);
        TileQuad Q;
        quad_mask(rc, lane, wid, mask, Q);
        __syncthreads();
        QuadCodes C;
        quad_codes(tab, mask, start, count, p0, a.tile_next[(uint64_t)f * T + tt], Q, C);
        const uint32_t x = wave_incl_scan(C.nb);
        if (lane == 63) wsum[wid] = x;
        __syncthreads();
        uint32_t wbase = 0, sbits = 0;
#pragma unroll
        for (int i = 0; i < PK_THREADS / 64; ++i) {
          const uint32_t ws = wsum[i];
          wbase += (i < wid) ? ws : 0u;
          sbits += ws;
        }
        if (C.nb) {
          unsigned long long pp = run + wbase + x - C.nb;
          quad_emit(tab, Q, C, [&](uint32_t val, uint32_t n) {
            const uint32_t b = (uint32_t)(pp & 31u);
            const uint64_t v = (uint64_t)val << ((64u - b - n) & 63u);
            if (n) {
              or_word(pp >> 5, (uint32_t)(v >> 32));
              or_word((pp >> 5) + 1, (uint32_t)v);
            }
            pp += n;
          });
        }
        run += sbits;
        __syncthreads();
      }
  }
}

// Each group's bits in the word holding its first bit (enc_pack and
// enc_pack_over leave them in tile_bits at the group's first tile), OR-ed into
// that word once every group has stored its own words.
__global__ __launch_bounds__(EDGES_THREADS) void enc_edges(EncArgs a) {
  const uint32_t T = a.tiles_per_frame;
  const uint32_t ng = (a.tile_hi - a.tile_lo + PACK_SUB - 1) / PACK_SUB;   // groups of the frame (band)
  for (uint32_t f = blockIdx.y; f < a.n_frames; f += gridDim.y) {
    if (a.frame_flags[f] & (FLAG_LONG | FLAG_BAD)) continue;
    uint32_t* out32 = reinterpret_cast<uint32_t*>(a.out + (uint64_t)f * a.out_stride);
    for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < ng; g += gridDim.x * 256) {
      const uint64_t t = (uint64_t)f * T + a.tile_lo + (uint64_t)g * PACK_SUB;
      const uint32_t e = a.tile_bits[t];
      if (e) atomicOr(&out32[a.tile_off[t] >> 5], __builtin_bswap32(e));
    }
  }
}

__global__ __launch_bounds__(ENC_WAVE_THREADS) void enc_tail(EncArgs a) {
  const uint32_t f = blockIdx.x * 64 + threadIdx.x;
  if (f >= a.n_frames) return;
  if ((uint64_t)a.W * a.H == 0) return;
  uint8_t* out = a.out + (uint64_t)f * a.out_stride;
  const uint64_t e0 = a.data_end[f];
  const uint64_t B = e0 >> 3;            // the partial byte (the reference's cache >> 24)
  const uint8_t P = (e0 & 7) ? out[B] : 0u;
  out[B] = P;
  out[B + 1] = P;
  out[B + 2] = 0;
  out[B + 3] = 0;
  out[B + 4] = 0;
  a.out_len[f] = B + 5;
}

// ---------------------------------------------------------------------------
// K6: frames with codes over FAST_MAX_CODE_BITS (FLAG_LONG).
//
// A write of an n-bit code at absolute stream bit p behaves like the
// reference's write_24bits (bitwriter.rs:55-73) with bit_offset = p & 7
// (the writer flushes every whole byte, so bit_offset is always the position
// mod 8 once the table header is out):
//  * (p & 7) + n <= 32: the code lands exactly on bits [p, p + n);
//  * otherwise `32 - bit_offset` wraps (u8) and the shift is masked to 5 bits:
//    the 32-bit window at byte p >> 3 becomes window + (code << ((32 - (p & 7)
//    - n) & 31)) mod 2^32 -- carries into the pending bits of the codes before
//    it included -- and every bit after the window up to p + n is zero (the
//    flush loop shifts the cache out).
// Phase 0 places the codes of the first kind (global atomicOr after the tile
// zeroes the words only it writes; enc_tilescan zeroed the shared ones).
// Phase 1 re-derives every symbol's position and applies the wrapped writes to
// their windows, whose earlier bits phase 0 has finalised.  Wrapped windows
// are disjoint: a window ends before its code's end (p + n > window + 32),
// and the next code starts there.  In band mode a window that starts in the
// byte holding band_bit0 also covers (and may carry into) the previous band's
// last bits: at most one per band (n >= 26), so it is recorded in the band's
// two trailer words (band_fix) and applied by enc_band_fix after the bands are
// merged.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void wrapped_write(uint8_t* out, uint64_t p, uint32_t v, uint32_t n) {
  const uint64_t B = p >> 3;
  const uint32_t bo = (uint32_t)(p & 7u);
  const uint32_t sh = (uint32_t)(uint8_t)(32u - (uint8_t)(bo + n)) & 31u;
  const uint32_t w = ((uint32_t)out[B] << 24) | ((uint32_t)out[B + 1] << 16) | ((uint32_t)out[B + 2] << 8) | out[B + 3];
  const uint32_t r = w + (v << sh);
  out[B] = (uint8_t)(r >> 24);
  out[B + 1] = (uint8_t)(r >> 16);
  out[B + 2] = (uint8_t)(r >> 8);
  out[B + 3] = (uint8_t)r;
}

__global__ __launch_bounds__(ENC_THREADS) void enc_pack_long(EncArgs a, int phase) {
  __shared__ uint32_t code[N_BINS];
  __shared__ uint32_t lens[N_BINS];
  __shared__ uint32_t mask[ENC_TILE / 32];
  __shared__ uint32_t wsum[ENC_THREADS / 64];
  if (!(a.frame_flags[a.n_frames] & FLAG_LONG)) return;   // no long-code frame in the batch
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t N = (int64_t)a.W * a.H;
  const int p0 = 4 * threadIdx.x;
  uint32_t cur_f = NONE;
  uint64_t t0, t1;
  tile_range(a, t0, t1);
  TileIter it(a, t0);
  for (uint64_t w = t0; w < t1; ++w, it.step(1)) {
    const uint32_t f = it.f, tt = it.tt();
    if ((a.frame_flags[f] & (FLAG_LONG | FLAG_BAD)) != FLAG_LONG) continue;   // block-uniform
    const uint64_t t = it.tile();
    const int64_t start = (int64_t)tt * ENC_TILE;
    const int count = (int)((N - start) < ENC_TILE ? (N - start) : ENC_TILE);
    uint32_t rc[4];
    quad_fetch(a, f, tt, p0, rc);
    __syncthreads();
    if (f != cur_f) {
      for (int b = threadIdx.x; b < N_BINS; b += ENC_THREADS) {
        code[b] = a.tbl_code[(uint64_t)f * N_BINS + b];
        lens[b] = a.tbl_len8[(uint64_t)f * N_BINS + b];
      }
      cur_f = f;
    }
    TileQuad Q;
    quad_mask(rc, lane, wid, mask, Q);
    __syncthreads();
    const uint32_t nb = quad_nbits(lens, mask, start, count, p0, a.tile_next[t], Q);
    const uint32_t x = wave_incl_scan(nb);
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    uint32_t wbase = 0, tile_bits = 0;
#pragma unroll
    for (int k = 0; k < ENC_THREADS / 64; ++k) {
      const uint32_t ws = wsum[k];
      wbase += (k < wid) ? ws : 0u;
      tile_bits += ws;
    }
    const uint64_t s0 = a.tile_off[t];
    uint8_t* out = a.out + (uint64_t)f * a.out_stride;
    uint32_t* out32 = reinterpret_cast<uint32_t*>(out);
    if (phase == 0) {
      const uint64_t e0 = s0 + tile_bits, w0 = s0 >> 5;
      const uint32_t nw = tile_bits ? (uint32_t)(((e0 + 31) >> 5) - w0) : 0u;
      for (uint32_t m = threadIdx.x; m < nw; m += ENC_THREADS) {
        const bool shared = (m == 0 && (s0 & 31)) || (m == nw - 1 && (e0 & 31));
        if (!shared) out32[w0 + m] = 0u;
      }
      __threadfence();
      __syncthreads();
    }
    uint64_t pos = s0 + wbase + x - nb;
    auto emit = [&](uint32_t bin) {
      const uint32_t n = lens[bin], v = code[bin];
      const uint32_t bo = (uint32_t)(pos & 7u);
      if (bo + n <= 32u) {
        if (phase == 0 && n) {
          const uint32_t o = (uint32_t)(pos & 31u);
          const uint64_t y = (uint64_t)v << (64u - o - n);
          atomicOr(&out32[pos >> 5], __builtin_bswap32((uint32_t)(y >> 32)));
          if (o + n > 32u) atomicOr(&out32[(pos >> 5) + 1], __builtin_bswap32((uint32_t)y));
        }
      } else if (phase == 1) {
        if (a.band && (pos & ~7ull) < a.band_bit0) {   // window reaches the previous band: deferred
          a.band_fix[0] = BAND_FIX_WRITE | ((uint32_t)(pos - a.band_bit0) << 8) | n;
          a.band_fix[1] = v;
        } else {
          wrapped_write(out, pos, v, n);
        }
      }
      pos += n;
    };
    uint32_t run[4];
    quad_runs(mask, start, count, p0, a.tile_next[t], Q, run);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t b[5];
      const uint32_t n = rec2_syms(Q.rc[q], b);
      for (uint32_t k = 0; k < n; ++k) emit(b[k]);
      if (run[q] > 0) {
        uint32_t m = run[q] - 1;
        while (true) {
          emit(BIN_PREFIX + P_RUN1 + (m & 7u));
          if (m < 8) break;
          m >>= 3;
        }
      }
    }
  }
}

}  // namespace nice

namespace nice {

// ---------------------------------------------------------------------------
// Band assembly (one image sharded over ranks): OR the bands' word arrays into
// the stream (header words are already there, zero padded), then the tail.
// band_w0[r]: first stream word of band r; band_off[r]: its first word in the
// concatenated array; band_off[R]: total words.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(BAND_THREADS) void enc_band_merge(uint32_t* out32, const uint32_t* words,
                                                      const unsigned long long* band_w0,
                                                      const unsigned long long* band_off, uint32_t R) {
  const uint32_t r = blockIdx.y;
  if (r >= R) return;
  const unsigned long long n = band_off[r + 1] - band_off[r];
  if (n < 3) return;
  const unsigned long long nd = n - 2;   // the last two words of a band are its trailer (enc_band_fix)
  const unsigned long long w0 = band_w0[r];
  const uint32_t* src = words + band_off[r];
  // 16 words per thread in flight: block b covers words [4096 b, 4096 (b + 1))
  constexpr int K = 16;
  const unsigned long long m0 = (unsigned long long)blockIdx.x * (256 * K) + threadIdx.x;
  if (m0 >= nd) return;
  uint32_t v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const unsigned long long m = m0 + 256ull * k;
    v[k] = m < nd ? src[m] : 0u;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const unsigned long long m = m0 + 256ull * k;
    if (m >= nd) break;
    if (m == 0 || m + 1 == nd) atomicOr(&out32[w0 + m], v[k]);   // shared with a neighbour or the header
    else out32[w0 + m] = v[k];
  }
}

// The deferred wrapped writes, band by band (their windows are disjoint; each
// reads the merged bits of the band before it).  One thread: at most R writes.
__global__ void enc_band_fix(uint8_t* out, const uint32_t* words, const unsigned long long* band_bit0,
                             const unsigned long long* band_off, uint32_t R, unsigned long long* bad) {
  if (threadIdx.x != 0) return;
  for (uint32_t r = 0; r < R; ++r) {
    const uint32_t f = words[band_off[r + 1] - 2];
    if (f & BAND_FIX_BAD) *bad = 1;   // packed with a wrong band_bits (enc_band_check)
    else if (f & BAND_FIX_WRITE) wrapped_write(out, band_bit0[r] + ((f >> 8) & 0xFFu), words[band_off[r + 1] - 1], f & 0xFFu);
  }
}

}  // namespace nice

namespace nice {

// Band helpers: first/last coded pixel of the band (over tiles [tile_lo,
// tile_hi) of frame 0), and the band's total data bits.
__global__ __launch_bounds__(BAND_THREADS) void enc_band_edges(EncArgs a, uint32_t* edges) {
  __shared__ uint32_t s_first, s_last;
  if (threadIdx.x == 0) { s_first = NONE; s_last = 0; }
  __syncthreads();
  uint32_t fi = NONE, la = 0;
  bool any = false;
  for (uint32_t t = a.tile_lo + threadIdx.x; t < a.tile_hi; t += 256) {
    fi = min(fi, a.tile_first[t]);
    if (a.tile_last[t] != NONE) { la = max(la, a.tile_last[t]); any = true; }
  }
  atomicMin(&s_first, fi);
  if (any) atomicMax(&s_last, la);
  __syncthreads();
  if (threadIdx.x == 0) {
    edges[0] = s_first;
    edges[1] = s_first == NONE ? NONE : s_last;
  }
}

// The band's data bits: its own symbol counts (bhist, 858 bins; the mode
// prefixes derived from the payload streams as enc_tables does) times the code
// lengths of the shared tables.  info = {bits, data start bit}.
// nice_band_pack_bits after nice_band_tables_dev: the band_bits argument must
// be the device count (d_info[0]); on a mismatch the band is flagged FLAG_BAD
// and the pack kernels write nothing (the flag is recomputed on every call)
__global__ void enc_band_check(EncArgs a, const unsigned long long* info, unsigned long long band_bits) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const bool bad = info[0] != band_bits;
    a.frame_flags[0] = (a.frame_flags[0] & ~FLAG_BAD) | (bad ? FLAG_BAD : 0u);
    if (bad) a.band_fix[0] = BAND_FIX_BAD;   // reported by nice_band_assemble
  }
}

__global__ __launch_bounds__(BAND_THREADS) void enc_band_sum(EncArgs a, const uint32_t* bhist, unsigned long long* info) {
  __shared__ unsigned long long s_bits;
  __shared__ uint32_t s_mode[5];
  if (threadIdx.x == 0) s_bits = 0;
  if (threadIdx.x < 5) s_mode[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long v = 0;
  uint32_t c[5] = {0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < N_BINS; b += 256) {
    const uint32_t h = bhist[b];
#pragma unroll
    for (int k = 0; k < 5; ++k) c[k] += mode_id_bin(k, b) ? h : 0u;
    if (b >= BIN_PREFIX && b < BIN_PREFIX + 5) continue;   // mode prefixes: below
    v += (unsigned long long)h * a.tbl_len8[b];
  }
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if (c[k]) atomicAdd(&s_mode[k], c[k]);
  atomicAdd(&s_bits, v);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long bits = s_bits;
    for (int k = 0; k < 5; ++k)
      bits += (unsigned long long)(s_mode[k] / mode_id_syms(k)) * a.tbl_len8[BIN_PREFIX + k];
    info[0] = bits;
    info[1] = a.seed_bit[0];
  }
}

}  // namespace nice
