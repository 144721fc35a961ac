// nice_encode.hip -- MI355X (gfx950) encoder for the NICE2 bitstream: what
// sits between the classify kernels (nice_classify.hip: per-pixel records,
// symbol histogram, per-tile first/last coded pixel) and the bit packers
// (nice_pack.hip), then the tail and the band assembly.  All kernels take the
// whole batch of same-shape frames.
//   enc_group_reduce, enc_tailruns
//                  the run of each tile's last coded pixel may cross tiles;
//                  resolve it with a suffix-min over tiles and add its base-8
//                  digits (code.rs:371-407) to the histogram.
//   enc_tables     one wave per (frame, stream): code lengths by exact replay of
//                  std BinaryHeap (hfe.rs:58-87), canonical codes (hfe.rs:255-296).
//   enc_header     one wave per frame: file header (code.rs:72-84) + table
//                  header (hfe.rs:97-103) bits, data start position.
//   enc_tail       per frame, after the packers: [P, P, 0, 0, 0] after the data
//                  (hfe.rs:115, code.rs:421-422) and the stream length.
//   enc_band_*     one image sharded over ranks: a band's edges and bit count,
//                  the merge of the bands' words and their deferred wrapped
//                  writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

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
// The tail, once the packers have written the data and its end bit.
// ---------------------------------------------------------------------------
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
