// nice_pack.hip -- the encoder's bit packers (MI355X, gfx950): everything
// between the code tables (enc_tables, nice_encode.hip) and the tail.
//   enc_packtab   per frame: the packer's code tables (nice_rec.hpp PackTab):
//                 each record slot -> {code, length}, T0 with the mode prefix
//                 composed in front, run digits composed per run length;
//                 FLAG_LONG for frames an entry of which exceeds 32 bits
//   enc_pack      per group of PACK_SUB tiles, one pass: the pixels' codes from
//                 three lookups each, a block scan of their lengths, the group's
//                 stream offset by a decoupled look-back over the preceding
//                 groups' status words (frames: from the data start; bands: from
//                 band_bit0), codes MSB-first into an LDS bit buffer
//                 (bitwriter.rs:55-73), then shifted to the offset and stored
//   enc_pack_over the groups over that buffer, OR-ed into the output directly
//   enc_edges     ORs each group's first partial word into the word the group
//                 before it (or the header) wrote
// FLAG_LONG frames (a code over FAST_MAX_CODE_BITS, or a composed entry over
// 32 bits) take enc_tilebits -> enc_tilescan -> enc_pack_long instead.
//
// The kernels are built from stages written once (DESIGN.md §4 has the stage x
// kernel table): the arithmetic in nice_pack.hpp (tile extent, run digits,
// rc_index, run after a pixel, span placement, wrapped window), what touches
// tables, LDS or a wave as the pack_* functions below.  Two sets of per-thread
// helpers sit on them: quad_* (4 pixels per thread, one 16-byte record load:
// enc_tilebits, enc_pack_over, enc_pack_long) and lane_* (16 pixels per lane,
// four loads: enc_pack).  The record loads and the code loops differ by that
// width and stay two functions each; no pack_* function asks who calls it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nice_enc_shared.hpp"
#include "nice_format.h"
#include "nice_kernels.h"
#include "nice_pack.hpp"
#include "nice_rec.hpp"

namespace nice {

// LDS bit buffer: <= NICE_PACK_CAP_BPP bits per pixel on average over a group
// (denser groups go to enc_pack_over)
constexpr int PACK_CAP_BITS = PACK_SUB * ENC_TILE * NICE_PACK_CAP_BPP;
constexpr int PACK_MAX_WORDS = PACK_CAP_BITS / 32 + 2;
constexpr int PACK_WAVES = PK_THREADS / 64;   // waves of a pack block, of every kernel here
static_assert(ENC_THREADS == PK_THREADS, "pack_block_prefix: one wave count");

// ---------------------------------------------------------------------------
// Stages every pack kernel shares.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint2 pt_entry(const PackTab& tab, uint32_t r, int i) {
  // 8-byte entries at the record's field offsets (nice_rec.hpp: bits 3..13,
  // 14..22, 23..31)
  const char* tb = reinterpret_cast<const char*>(&tab);
  return i == 0 ? *reinterpret_cast<const uint2*>(tb + offsetof(PackTab, t0) + (r & 0x3FF8u))
       : i == 1 ? *reinterpret_cast<const uint2*>(tb + offsetof(PackTab, t1) + ((r >> 11) & 0xFF8u))
                : *reinterpret_cast<const uint2*>(tb + offsetof(PackTab, t2) + ((r >> 20) & 0xFF8u));
}

// The frame's PackTab into LDS (a barrier before its first use).
__device__ __forceinline__ void pack_load_tab(PackTab& tab, const EncArgs& a, uint32_t f, int tid) {
  const uint4* src = reinterpret_cast<const uint4*>(a.packtab + (uint64_t)f * sizeof(PackTab));
  uint4* dst = reinterpret_cast<uint4*>(&tab);
  for (int i = tid; i < (int)(sizeof(PackTab) / 16); i += PK_THREADS) dst[i] = src[i];
}

// A pixel's codes (T0, T1, T2 of record r, run entry rci) composed into one
// value, exact when their total t <= 32 (the shifts stay below 32 then).
__device__ __forceinline__ uint32_t pack_compose(const PackTab& tab, uint32_t r, uint32_t rci, uint32_t& t) {
  const uint2 e0 = pt_entry(tab, r, 0), e1 = pt_entry(tab, r, 1), e2 = pt_entry(tab, r, 2);
  const uint2 e3 = tab.rc[rci];
  t = e0.y + e1.y + e2.y + e3.y;
  uint32_t v = e0.x;
  v = (v << (e1.y & 31u)) | e1.x;
  v = (v << (e2.y & 31u)) | e2.x;
  v = (v << (e3.y & 31u)) | e3.x;
  asm volatile("" : "+v"(v) : "v"(t));   // materialise the pixel's code now (no entries kept live)
  return v;
}

// The same codes entry by entry through put(val, n) (each entry <= 32 bits:
// longer ones make the frame FLAG_LONG), then a long run's further digits.
template <class Put>
__device__ __forceinline__ void pack_put_entries(const PackTab& tab, uint32_t r, uint32_t run, Put&& put) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const uint2 e = pt_entry(tab, r, i);
    put(e.x, e.y);
  }
  const uint2 e3 = tab.rc[rc_index(run)];
  put(e3.x, e3.y);
  pack_run_digits_past2(run, [&](uint32_t d) {
    const uint2 e = tab.rc[d];
    put(e.x, e.y);
  });
}

// fn(bin) for every symbol of a pixel in emission order (full code tables: the
// long path): the record's symbols, then the digits of the run after it.
template <class Fn>
__device__ __forceinline__ void pack_pixel_bins(uint32_t rec, uint32_t run, Fn&& fn) {
  uint32_t b[5];
  const uint32_t n = rec2_syms(rec, b);
  for (uint32_t k = 0; k < n; ++k) fn(b[k]);
  if (run > 0) pack_run_digits(run, [&](uint32_t d) { fn(BIN_PREFIX + P_RUN1 + d); });
}

// Block prefix from the waves' inclusive totals (wsum, written by lane 63 of
// each wave before a barrier): the bits of the waves before wave wid; total:
// the block's.
__device__ __forceinline__ uint32_t pack_block_prefix(const uint32_t* wsum, int wid, uint32_t& total) {
  uint32_t wbase = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < PACK_WAVES; ++i) {
    const uint32_t ws = wsum[i];
    wbase += (i < wid) ? ws : 0u;
    total += ws;
  }
  return wbase;
}

// ---------------------------------------------------------------------------
// quad_*: a thread owns 4 consecutive pixels of a tile and reads their records
// with one 16-byte load.
// ---------------------------------------------------------------------------
struct TileQuad {
  uint32_t rc[4];
  uint32_t nib;        // coded flags of the 4 pixels
};

// The thread's 4 records of tile te of frame f (run members past the frame end).
__device__ __forceinline__ void quad_fetch(const EncArgs& a, uint32_t f, const TileExtent& te, int p0, uint32_t (&rc)[4]) {
  const uint32_t* rp = a.recs + (uint64_t)f * a.rec_stride + te.start + p0;
  if (p0 + 3 < te.count) {
    const uint4 v = *reinterpret_cast<const uint4*>(rp);
    rc[0] = v.x; rc[1] = v.y; rc[2] = v.z; rc[3] = v.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) rc[q] = (p0 + q < te.count) ? rp[q] : rec2_unc(0);
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
__device__ __forceinline__ void quad_runs(const uint32_t* mask, const TileExtent& te, int p0, uint32_t next_tile_px,
                                          const TileQuad& Q, uint32_t (&run)[4]) {
  const int nx_local = next_coded_local(mask, p0 + 3);
  const uint32_t s32 = (uint32_t)te.start + (uint32_t)p0;
  const uint32_t after = (nx_local < te.count) ? (uint32_t)te.start + (uint32_t)nx_local : next_tile_px;
#pragma unroll
  for (int q = 0; q < 4; ++q) run[q] = pack_run_after(Q.nib, q, s32, after);
}

__device__ __forceinline__ void load_lens(uint32_t* lens, const EncArgs& a, uint32_t f) {
  for (int b = threadIdx.x; b < N_BINS; b += ENC_THREADS) lens[b] = a.tbl_len8[(uint64_t)f * N_BINS + b];
}

// Bits of the thread's 4 pixels (prefix, payload, run digits) from full code
// lengths (any length).
__device__ __forceinline__ uint32_t quad_nbits(const uint32_t* lens, const TileQuad& Q, const uint32_t (&run)[4]) {
  uint32_t nb = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) pack_pixel_bins(Q.rc[q], run[q], [&](uint32_t bin) { nb += lens[bin]; });
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
  __shared__ uint32_t wsum[PACK_WAVES];
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
    const uint32_t f = it.f;
    if (!long_path(a, f)) continue;   // block-uniform
    const TileExtent te = pack_tile_extent(N, it.tt());
    uint32_t rc[4];
    quad_fetch(a, f, te, p0, rc);
    __syncthreads();
    if (f != cur_f) { load_lens(tbl, a, f); cur_f = f; }
    TileQuad Q;
    quad_mask(rc, lane, wid, mask, Q);
    __syncthreads();
    uint32_t run[4];
    quad_runs(mask, te, p0, a.tile_next[t], Q, run);
    const uint32_t x = wave_incl_scan(quad_nbits(tbl, Q, run));
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    uint32_t tile_bits;
    pack_block_prefix(wsum, wid, tile_bits);
    if (threadIdx.x == 0) a.tile_bits[t] = tile_bits;
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
// run after it, and the thread's total.
struct QuadCodes {
  uint32_t v[4], tot[4], run[4], nb, tmax;
};
__device__ __forceinline__ void quad_codes(const PackTab& tab, const uint32_t* mask, const TileExtent& te, int p0,
                                           uint32_t next_tile_px, const TileQuad& Q, QuadCodes& C) {
  quad_runs(mask, te, p0, next_tile_px, Q, C.run);
  C.nb = 0;
  C.tmax = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    C.v[q] = pack_compose(tab, Q.rc[q], rc_index(C.run[q]), C.tot[q]);
    C.tmax = max(C.tmax, C.tot[q]);
    C.nb += C.tot[q];
    // run digits past a long run's first two (runs of >= 65)
    pack_run_digits_past2(C.run[q], [&](uint32_t d) { C.nb += tab.rc[d].y; });
  }
}
// Every code of the thread's pixels, in order, through put(val, n) (n <= 32
// bits of val, 0 when n == 0): one put per pixel when every pixel of the wave
// fits 32 bits (the common case), else one per entry.
template <class Put>
__device__ __forceinline__ void quad_emit(const PackTab& tab, const TileQuad& Q, const QuadCodes& C, Put&& put) {
  if (__all(C.tmax <= 32u)) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      put(C.v[q], C.tot[q]);
      pack_run_digits_past2(C.run[q], [&](uint32_t d) {
        const uint2 e = tab.rc[d];
        put(e.x, e.y);
      });
    }
  } else {
    for (int q = 0; q < 4; ++q) pack_put_entries(tab, Q.rc[q], C.run[q], put);
  }
}

// ---------------------------------------------------------------------------
// lane_*: a lane owns 16 consecutive pixels of a tile (enc_pack).
// ---------------------------------------------------------------------------
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

// The lane's 16 records of tile te of frame f.
__device__ __forceinline__ void lane_recs(const EncArgs& a, uint32_t f, const TileExtent& te, int lane,
                                          uint32_t (&rec)[PW_PX]) {
  const int p0 = PW_PX * lane;
  const uint32_t* rp = a.recs + (uint64_t)f * a.rec_stride + te.start + p0;
  if (p0 + PW_PX <= te.count) {
#pragma unroll
    for (int q = 0; q < PW_PX / 4; ++q) {
      const uint4 r = reinterpret_cast<const uint4*>(rp)[q];
      rec[4 * q] = r.x; rec[4 * q + 1] = r.y; rec[4 * q + 2] = r.z; rec[4 * q + 3] = r.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < PW_PX; ++q) rec[q] = (p0 + q < te.count) ? rp[q] : rec2_unc(0);
  }
}
// The lane's 16 pixels of tile te of frame f: each pixel's composed code and
// length, the lane's bit count.  Pixel indices are < 2^30 (the boundary's
// frame cap): 32-bit arithmetic.
// cmw: the tile's coded-flag words in the standard order (enc_rundigits wrote
// them; 16 bits per lane) when the frame's classify produced them, else null
// (bands, the window kernels): then the flags come from the records.
__device__ __forceinline__ void lane_codes(const EncArgs& a, const PackTab& tab, uint32_t f, const TileExtent& te,
                                           uint32_t next_tile_px, int lane, const uint32_t (&rec)[PW_PX], LanePx& P,
                                           const uint32_t* cmw) {
  const int p0 = PW_PX * lane;
  P.rp = a.recs + (uint64_t)f * a.rec_stride + te.start + p0;
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
  P.s = (uint32_t)te.start + (uint32_t)p0;
  P.after = nl < 64 ? (uint32_t)te.start + nf : next_tile_px;
  P.nb = 0;
  P.tmax = 0;
  P.rmax = 0;
  // each pixel's run-code index, from the last pixel back: the next coded
  // pixel is carried in a register instead of a bit scan per pixel (the
  // carried form of pack_run_after)
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
    uint32_t t;
    P.v[q] = pack_compose(tab, rec[q], rci[q], t);
    P.tot4[q >> 2] |= t << (8 * (q & 3));
    P.tmax = max(P.tmax, t);
    P.nb += t;
  }
  if (P.rmax > 64u) {   // run digits past a long run's first two (runs of >= 65)
    for (int q = 0; q < PW_PX; ++q)
      pack_run_digits_past2(pack_run_after(P.cm, q, P.s, P.after), [&](uint32_t d) { P.nb += tab.rc[d].y; });
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
    // entry by entry from the records again
    for (int q = 0; q < PW_PX; ++q) {
      if ((P.cm >> q) & 1u)   // coded (P.cm has no bits past the frame's end)
        pack_put_entries(tab, P.rp[q], pack_run_after(P.cm, q, P.s, P.after), put);
    }
  }
  if (n) atomicOr(wp, (uint32_t)(acc << (32u - n)));
}

__global__ __launch_bounds__(PK_THREADS, PACK_BLOCKS_PER_CU) void enc_pack(EncArgs a) {
  __shared__ PackTab tab;
  __shared__ uint32_t bits[PACK_MAX_WORDS];
  __shared__ uint32_t wsum[PACK_WAVES];
  __shared__ uint32_t s_f, s_k;
  __shared__ unsigned long long s_off;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t nt = a.tile_hi - a.tile_lo;
  const uint32_t ng = (nt + PACK_SUB - 1) / PACK_SUB;   // groups per frame
  const uint32_t T = a.tiles_per_frame;
  const uint32_t I = a.pack_slots, slot = blockIdx.x % a.pack_slots;
  uint32_t cf = NONE, ck = 0, seq = 0;   // wave 0's work cursor
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
      pack_load_tab(tab, a, f, tid);
      cur_f = f;
    }
    for (uint32_t i = tid; i < used_words; i += PK_THREADS) bits[i] = 0;
    __syncthreads();   // the frame's tables in LDS, the buffer clear
    // wave wid: tile tt0 + wid of the group
    LanePx P;
    uint32_t x = 0;
    const bool mine = (uint32_t)wid < nsub;   // wave-uniform
    if (mine) {
      const TileExtent te = pack_tile_extent((int64_t)a.W * a.H, tt0 + wid);
      lane_recs(a, f, te, lane, rec);
      lane_codes(a, tab, f, te, a.tile_next[(uint64_t)f * T + tt0 + wid], lane, rec, P,
                 a.cmask_std ? a.cmask + ((uint64_t)f * T + tt0 + wid) * (ENC_TILE / 32) : nullptr);
      x = wave_incl_scan(P.nb);
    }
    if (lane == 63) wsum[wid] = mine ? x : 0u;
    __syncthreads();
    uint32_t gbits;   // the group's bits; wbase: those before this wave's tile
    const uint32_t wbase = pack_block_prefix(wsum, wid, gbits);
    // (waves ranked by their bits at priorities 3..0 for the puts: no
    // faster, r06zv_ab_pack_place.log)
    const bool over = gbits > a.pack_cap_bits;   // block-uniform
    // the group's count goes out before the puts: the look-backs of the
    // groups after it wait on it (a look-back was ~40 % of a group's time)
    const bool agg_out = g > 0;
    if (agg_out && tid == 0) st_store(&a.status[f * ng + g], ST_AGG | gbits);
    if (!over && mine && P.nb) lane_emit(tab, P, bits, wbase + x - P.nb);
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
    // place the group's bits at its stream offset
    const unsigned long long s0 = s_off;
    const BitSpan sp = pack_span(s0, gbits);
    uint32_t* out32 = reinterpret_cast<uint32_t*>(a.out + (uint64_t)f * a.out_stride);
    if (!over) {
      for (uint32_t m = tid; m < sp.nw; m += PK_THREADS) {
        const uint32_t hi = m ? bits[m - 1] : 0u;
        const uint32_t lo = bits[m];   // zero past the group's bits
        const uint32_t v = sp.sh ? (uint32_t)((((uint64_t)hi << 32) | lo) >> sp.sh) : lo;
        // a word is stored by the group holding its first bit (zeros past
        // the group's end); this group's bits in the word holding its
        // start go to enc_edges
        if (pack_span_first_shared(sp, m)) a.tile_bits[t0] = v;
        else out32[sp.w0 + m] = __builtin_bswap32(v);
      }
    } else if (tid == 0) {
      // over the LDS buffer: listed for enc_pack_over (after this kernel, before enc_edges)
      const uint32_t k = atomicAdd(a.over_count, 1u);
      a.over_list[k] = make_uint2(f * ng + g, gbits);
    }
    if (tid == 0) {
      a.tile_off[t0] = s0;
      if (over || !(sp.nw && sp.sh)) a.tile_bits[t0] = 0u;
      if (tt0 + nsub == T) a.data_end[f] = s0 + gbits;
    }
    used_words = over ? 0u : sp.nw + 1;   // an over-cap group writes nothing into the buffer
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
  }
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
  __shared__ uint32_t wsum[PACK_WAVES];
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
    pack_load_tab(tab, a, f, tid);
    const unsigned long long s0 = a.tile_off[t0];
    const BitSpan sp = pack_span(s0, gbits);
    uint32_t* out32 = reinterpret_cast<uint32_t*>(a.out + (uint64_t)f * a.out_stride);
    // zero the words only this group writes (every word whose first bit is
    // the group's), then OR each code into place, tile by tile
    for (uint32_t m = tid; m < sp.nw; m += PK_THREADS)
      if (!pack_span_first_shared(sp, m)) out32[sp.w0 + m] = 0u;
    if (tid == 0) a.tile_bits[t0] = 0u;
    __threadfence();
    __syncthreads();
    auto or_word = [&](uint64_t wd, uint32_t v) {
      if (!v) return;
      if (sp.sh && wd == sp.w0) atomicOr(&a.tile_bits[t0], v);
      else atomicOr(&out32[wd], __builtin_bswap32(v));
    };
    unsigned long long run = s0;
    for (uint32_t s = 0; s < nsub; ++s) {
      const uint32_t tt = tt0 + s;
      const TileExtent te = pack_tile_extent(N, tt);
      quad_fetch(a, f, te, p0, rc);
      TileQuad Q;
      quad_mask(rc, lane, wid, mask, Q);
      __syncthreads();
      QuadCodes C;
      quad_codes(tab, mask, te, p0, a.tile_next[(uint64_t)f * T + tt], Q, C);
      const uint32_t x = wave_incl_scan(C.nb);
      if (lane == 63) wsum[wid] = x;
      __syncthreads();
      uint32_t sbits;
      const uint32_t wbase = pack_block_prefix(wsum, wid, sbits);
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

// ---------------------------------------------------------------------------
// Long codes: frames with codes over FAST_MAX_CODE_BITS (FLAG_LONG).
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
//    flush loop shifts the cache out): pack_wrapped_window, wrapped_write.
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
__global__ __launch_bounds__(ENC_THREADS) void enc_pack_long(EncArgs a, int phase) {
  __shared__ uint32_t code[N_BINS];
  __shared__ uint32_t lens[N_BINS];
  __shared__ uint32_t mask[ENC_TILE / 32];
  __shared__ uint32_t wsum[PACK_WAVES];
  if (!(a.frame_flags[a.n_frames] & FLAG_LONG)) return;   // no long-code frame in the batch
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t N = (int64_t)a.W * a.H;
  const int p0 = 4 * threadIdx.x;
  uint32_t cur_f = NONE;
  uint64_t t0, t1;
  tile_range(a, t0, t1);
  TileIter it(a, t0);
  for (uint64_t w = t0; w < t1; ++w, it.step(1)) {
    const uint32_t f = it.f;
    if (!long_path(a, f)) continue;   // block-uniform
    const uint64_t t = it.tile();
    const TileExtent te = pack_tile_extent(N, it.tt());
    uint32_t rc[4];
    quad_fetch(a, f, te, p0, rc);
    __syncthreads();
    if (f != cur_f) {
      for (int b = threadIdx.x; b < N_BINS; b += ENC_THREADS) code[b] = a.tbl_code[(uint64_t)f * N_BINS + b];
      load_lens(lens, a, f);
      cur_f = f;
    }
    TileQuad Q;
    quad_mask(rc, lane, wid, mask, Q);
    __syncthreads();
    uint32_t run[4];
    quad_runs(mask, te, p0, a.tile_next[t], Q, run);
    const uint32_t nb = quad_nbits(lens, Q, run);
    const uint32_t x = wave_incl_scan(nb);
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    uint32_t tile_bits;
    const uint32_t wbase = pack_block_prefix(wsum, wid, tile_bits);
    const uint64_t s0 = a.tile_off[t];
    uint8_t* out = a.out + (uint64_t)f * a.out_stride;
    uint32_t* out32 = reinterpret_cast<uint32_t*>(out);
    if (phase == 0) {
      // zero the words only this tile writes (enc_tilescan zeroed the shared ones)
      const BitSpan sp = pack_span(s0, tile_bits);
      for (uint32_t m = threadIdx.x; m < sp.nw; m += ENC_THREADS)
        if (!pack_span_first_shared(sp, m) && !pack_span_last_shared(sp, m)) out32[sp.w0 + m] = 0u;
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
#pragma unroll
    for (int q = 0; q < 4; ++q) pack_pixel_bins(Q.rc[q], run[q], emit);
  }
}

}  // namespace nice
