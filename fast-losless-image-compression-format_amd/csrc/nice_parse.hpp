// nice_parse.hpp -- the decoder's parse machinery (device code; included by
// nice_decode.hip only): the lane bit reader over its LDS ring, the table
// lookups, one pixel event on the general and on the fast parse, the kept
// events' layout and the routing of a slice between dec_emit and dec_place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nice.h"
#include "nice_bits.hpp"
#include "nice_dec_rec.hpp"
#include "nice_dec_state.hpp"
#include "nice_format.h"
#include "nice_kernels.h"

namespace nice {

// chunk geometry: chunk j of frame f covers bits [D + j*CB, D + (j+1)*CB)
__device__ __forceinline__ uint32_t n_chunks(uint64_t len, uint64_t D, uint32_t cb) {
  const uint64_t bits = len * 8;
  return bits > D ? (uint32_t)((bits - D + cb - 1) / cb) : 0u;
}

// ---------------------------------------------------------------------------
// Parse machinery of the four parse kernels (dec_sync, dec_sync_settle,
// dec_strict_refill, dec_emit).
//
// A lane parses one slice of the data bits.  It reads them from a private ring
// of RING_W big-endian words in LDS, refilled for the whole wave at once with
// 16-byte loads (consecutive lanes load consecutive 16 bytes of one ring), so
// the stream is read from HBM in whole lines.  The first-level LUTs and the
// canonical order for long codes live in LDS.
//
// The parse advances one pixel event per step: a prefix symbol, then -- for a
// coded pixel -- the mode's fixed payload sequence (code.rs:576-644): BACK_REF
// k; RGB r g b; LUMA ref, g, r, b; SMALL_DIFF index; LUMA2 g r b.  Slices
// therefore begin and end at prefix positions: a slice's parse stops at the
// first prefix at or after its end bit, which is where the next slice starts.
// ---------------------------------------------------------------------------
#ifndef NICE_RING_W
#define NICE_RING_W 20
#endif
constexpr uint32_t RING_W = NICE_RING_W;   // words per lane ring (a multiple of 4, >= 12)
constexpr uint32_t RING_STRIDE = RING_W;   // 16-byte aligned rings
static_assert(RING_W % 4 == 0 && RING_W >= 12, "ring size");
#ifdef NICE_PARSE_WPE
#define PARSE_ATTR __attribute__((amdgpu_waves_per_eu(NICE_PARSE_WPE)))
#else
#define PARSE_ATTR
#endif
constexpr uint32_t RING_QUADS = RING_W / 4;
constexpr uint32_t PIXEL_WORDS = 5;    // one pixel event: <= 5 symbols of <= 31 bits
// a checkpoint lies at the first prefix at or past its bit of the slice: less
// than one event past the slice's end
static_assert(DEC_MAX_CHUNK_BITS + PIXEL_WORDS * 32 <= (1u << CK_POS_BITS), "checkpoint position field");

constexpr uint32_t PFX_STREAM = S_PREFIX;
// payload stream i of mode m (code.rs:576-644), 4 bits each at 4 * (4m + i)
constexpr unsigned long long PAY_STREAMS =
    ((unsigned long long)S_BACK_REF << 0) |
    ((unsigned long long)S_RGB << 16) | ((unsigned long long)S_RGB << 20) | ((unsigned long long)S_RGB << 24) |
    ((unsigned long long)S_LUMA_REF << 32) | ((unsigned long long)S_LUMA_BASE << 36) |
    ((unsigned long long)S_LUMA_OTHER << 40) | ((unsigned long long)S_LUMA_OTHER << 44) |
    ((unsigned long long)S_SMALL_DIFF << 48);   // mode 4 (LUMA2): pay_stream
static_assert(P_BACK_REF == 0 && P_RGB == 1 && P_LUMA == 2 && P_SMALL_DIFF == 3 && P_LUMA2 == 4 &&
                  P_RUN1 == 5, "prefix numbering");
__device__ __forceinline__ uint32_t pay_stream(uint32_t m, uint32_t i) {
  // mode 4 (LUMA2) does not fit the 64-bit table: handled here
  return m == (uint32_t)P_LUMA2 ? (uint32_t)S_LUMA2_BASE + i : (uint32_t)(PAY_STREAMS >> (4u * (4u * m + i))) & 15u;
}

struct LutLds {
  uint16_t lut[DEC_LUT_BUDGET];
  uint32_t lo[N_BINS];   // canonical order (long codes): aligned lower bounds,
  uint16_t sym[N_BINS];  // symbols and lengths
  uint8_t len[N_BINS];
  uint32_t gp[16];    // per stream: lut_off | lut_bits << 16 | max_aob << 24
  uint32_t gs[16];    // per stream: canonical-order base | alphabet size << 16
  uint4 pp[8];        // fast parse: per prefix 0..4, the fast_param of its payload streams 0..3,
                      // and in bits 5..9 (which a lookup ignores) the symbol's place in the event word
};

__device__ inline void load_lut(LutLds& S, const DecTables* T) {
  const uint4* s = reinterpret_cast<const uint4*>(T->lut);
  uint4* d = reinterpret_cast<uint4*>(S.lut);
  for (uint32_t i = threadIdx.x; i < sizeof(S.lut) / 16; i += blockDim.x) d[i] = s[i];
  for (uint32_t i = threadIdx.x; i < N_BINS; i += blockDim.x) {
    S.lo[i] = T->lo[i];
    S.sym[i] = T->sym[i];
    S.len[i] = T->len[i];
  }
  if (threadIdx.x < N_STREAMS) {
    const int st = (int)threadIdx.x;
    S.gp[st] = (uint32_t)T->lut_off[st] | ((uint32_t)T->lut_bits[st] << 16) | ((uint32_t)T->max_aob[st] << 24);
    S.gs[st] = (uint32_t)stream_base(st) | ((uint32_t)stream_size(st) << 16);
  }
  if (threadIdx.x < 8u) {   // payload streams of each mode (code.rs:576-644), as fast parameters
    const uint32_t m = threadIdx.x;
    uint32_t w[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t st = m < 5u ? pay_stream(m, i) : 0u;
      w[i] = (32u - T->lut_bits[st]) | (ev_shift(m, i) << 5) | ((uint32_t)T->lut_off[st] << 17);
    }
    S.pp[m] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

__device__ __forceinline__ uint32_t stream_word(const uint8_t* p, uint64_t len, uint32_t w) {
  uint32_t v = 0;
  for (int k = 0; k < 4; ++k) {
    const uint64_t i = (uint64_t)w * 4 + k;
    v = (v << 8) | (i < len ? p[i] : (len ? p[len - 1] : 0u));   // stale last byte past the end
  }
  return v;
}

// Lane bit reader over its LDS ring: a left-aligned 64-bit window (next bit at
// bit 63) holding `avail` >= 32 valid bits between symbols.
struct Lane {
  unsigned long long pos;   // absolute bit position in the frame's stream
  unsigned long long win;
  uint32_t avail;
  uint32_t rp;              // next ring word to shift in
  uint32_t ws;              // fast parse: stream word held in ring word 0
};
// one more pixel event fits in the ring
__device__ __forceinline__ bool lane_ok(const Lane& L) { return L.rp + PIXEL_WORDS <= RING_W; }

__device__ __noinline__ void ring_fill_slow(uint32_t* dst, const uint8_t* p, uint64_t len, uint32_t w) {
  dst[0] = stream_word(p, len, w);
  dst[1] = stream_word(p, len, w + 1);
  dst[2] = stream_word(p, len, w + 2);
  dst[3] = stream_word(p, len, w + 3);
}
// Wave-cooperative refill: every lane's ring restarts at the word holding its
// position (rounded down to 16 bytes).  Must be reached by all 64 lanes.
// ws: the (16-byte aligned) stream word each lane's ring restarts at.
__device__ __forceinline__ void ring_fill_ws(uint32_t* wring, const uint8_t* p, uint64_t len, bool al16,
                                             uint32_t ws) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t full_words = al16 ? (len >> 2) : 0;   // words fully inside the stream
  uint4 v[RING_QUADS];
  uint32_t wq[RING_QUADS];
#pragma unroll
  for (uint32_t r = 0; r < RING_QUADS; ++r) {   // issue every load before waiting on any
    const uint32_t i = lane + 64u * r;
    const uint32_t owner = i / RING_QUADS, q = i - owner * RING_QUADS;
    wq[r] = (uint32_t)__shfl((int)ws, (int)owner) + 4u * q;   // all lanes: before any branch
    const uint64_t wl = (uint64_t)wq[r] + 4 <= full_words ? wq[r] : 0u;
    v[r] = *reinterpret_cast<const uint4*>(p + wl * 4);
  }
#pragma unroll
  for (uint32_t r = 0; r < RING_QUADS; ++r) {
    const uint32_t i = lane + 64u * r;
    const uint32_t owner = i / RING_QUADS, q = i - owner * RING_QUADS;
    uint32_t* dst = wring + owner * RING_STRIDE + 4u * q;
    if ((uint64_t)wq[r] + 4 <= full_words) {
      *reinterpret_cast<uint4*>(dst) = make_uint4(__builtin_bswap32(v[r].x), __builtin_bswap32(v[r].y),
                                                  __builtin_bswap32(v[r].z), __builtin_bswap32(v[r].w));
    } else {
      ring_fill_slow(dst, p, len, wq[r]);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}
template <bool FAST = false>
__device__ __forceinline__ void ring_fill(uint32_t* wring, const uint8_t* p, uint64_t len, bool al16,
                                          Lane& L) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t ws = (uint32_t)(L.pos >> 5) & ~3u;
  ring_fill_ws(wring, p, len, al16, ws);
  if constexpr (FAST) {
    L.ws = ws;
  } else {
    const uint32_t* my = wring + lane * RING_STRIDE;
    const uint32_t o = (uint32_t)(L.pos >> 5) - ws;
    const uint32_t sh = (uint32_t)(L.pos & 31u);
    L.win = (((unsigned long long)my[o] << 32) | my[o + 1]) << sh;
    L.avail = 64u - sh;
    L.rp = o + 2u;
  }
}

// Fast parse (DecTables::fast): the event's 64 bits are taken from the ring at
// its start and every symbol is one table lookup -- no long codes, no top-up.
__device__ __forceinline__ bool lane_ok_fast(const Lane& L) {
  return ((uint32_t)(L.pos >> 5) - L.ws) + 3u <= RING_W;
}
// Fast-path stream parameter: (32 - table width) | 2 * table offset << 16, so a
// lookup's byte address is ((v >> shift) << 17 + param) >> 16 (shifts use the
// low 5 bits of their operand; bits 5..15 do not reach the address, and S.pp
// keeps the symbol's event-word shift in bits 5..9: ev_shift).
__device__ __forceinline__ uint32_t fast_param(uint32_t gp) {
  return (32u - ((gp >> 16) & 31u)) | ((gp & 0xFFFFu) << 17);
}
__device__ __forceinline__ uint32_t fsym(unsigned long long& win, uint32_t& tot, const LutLds& S, uint32_t fp) {
  const uint32_t v = (uint32_t)(win >> 32);
  const uint32_t byte = (((v >> (fp & 31u)) << 17) + fp) >> 16;
  const uint32_t e = *reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(S.lut) + byte);
  const uint32_t n = e & 31u;
  win <<= n;
  tot += n;
  return e >> 5;
}

// Long code (longer than the LUT width): search of the canonical order.
__device__ __forceinline__ uint32_t long_code(const LutLds& S, uint32_t v, uint32_t gp, uint32_t gsz) {
  const uint32_t x = v >> (32u - (gp >> 24));
  int lo = (int)(gsz & 0xFFFFu), hi = lo + (int)(gsz >> 16) - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (S.lo[mid] <= x) hi = mid;
    else lo = mid + 1;
  }
  return ((uint32_t)S.sym[lo] << 5) | (uint32_t)S.len[lo];
}

// One symbol of stream st (gp: S.gp[st], passed in for the prefix stream,
// which a lane reads at every event).
__device__ __forceinline__ uint32_t dsym_gp(Lane& L, const uint32_t* my, const LutLds& S, uint32_t st,
                                            uint32_t gp) {
  const uint32_t v = (uint32_t)(L.win >> 32);
  uint32_t e = S.lut[(gp & 0xFFFFu) + (v >> (32u - ((gp >> 16) & 31u)))];
  if ((e & 31u) == 0) e = long_code(S, v, gp, S.gs[st]);
  const uint32_t n = e & 31u;
  L.pos += n;
  L.win <<= n;
  L.avail -= n;
  // top up to >= 32 bits (branch-free; lane_ok() guarantees the word exists)
  const uint32_t w = my[min(L.rp, RING_W - 1u)];
  const bool need = L.avail < 32u;
  L.win |= need ? ((unsigned long long)w << (32u - L.avail)) : 0ull;
  L.rp += need ? 1u : 0u;
  L.avail += need ? 32u : 0u;
  return e >> 5;
}
// One pixel event at a prefix position: the prefix and, for a coded pixel, its
// payload symbols.  Returns the prefix; s0..s3 receive the payload.
// The frame's stream parameters (S.gp) held in scalar registers: a payload
// symbol's parameters are selected by the prefix instead of read from LDS, so
// its LUT lookup does not wait on a dependent LDS read.
struct StreamParams {
  uint32_t g[N_STREAMS];
  __device__ __forceinline__ void load(const LutLds& S) {
#pragma unroll
    for (int i = 0; i < N_STREAMS; ++i) g[i] = __builtin_amdgcn_readfirstlane(S.gp[i]);
  }
};
__device__ __forceinline__ uint32_t pixel_event(Lane& L, const uint32_t* my, const LutLds& S,
                                                const StreamParams& G, uint32_t& s0, uint32_t& s1, uint32_t& s2,
                                                uint32_t& s3) {
  const uint32_t pfx = dsym_gp(L, my, S, PFX_STREAM, G.g[PFX_STREAM]);
  if (pfx < (uint32_t)P_RUN1) {
    const bool rgb = pfx == (uint32_t)P_RGB, lu = pfx == (uint32_t)P_LUMA, l2 = pfx == (uint32_t)P_LUMA2;
    const uint32_t gp0 = pfx == (uint32_t)P_BACK_REF ? G.g[S_BACK_REF] : rgb ? G.g[S_RGB] : lu ? G.g[S_LUMA_REF]
                       : l2 ? G.g[S_LUMA2_BASE] : G.g[S_SMALL_DIFF];
    s0 = dsym_gp(L, my, S, pay_stream(pfx, 0), gp0);
    if (rgb || lu || l2) {
      s1 = dsym_gp(L, my, S, pay_stream(pfx, 1), rgb ? G.g[S_RGB] : lu ? G.g[S_LUMA_BASE] : G.g[S_LUMA2_R]);
      s2 = dsym_gp(L, my, S, pay_stream(pfx, 2), rgb ? G.g[S_RGB] : lu ? G.g[S_LUMA_OTHER] : G.g[S_LUMA2_B]);
      if (lu) s3 = dsym_gp(L, my, S, S_LUMA_OTHER, G.g[S_LUMA_OTHER]);
    }
  }
  return pfx;
}

// pixel_event on the fast path: one 64-bit window per event (DecTables::fast
// bounds every event by 64 bits), taken at ring word o, bit sh of it (the
// relative-position loops); returns the prefix and the event's bit count in
// tot.  The mode's payload parameters come in one LDS read (selecting them from
// scalar registers by prefix took a move and a select per candidate).  EV: also the
// coded pixel's event word (ev_pack), each symbol shifted to its place by the
// shift its parameter word carries -- off the chain of dependent lookups.
template <bool EV = false>
__device__ __forceinline__ uint32_t pixel_event_fast_at(const uint32_t* my, const LutLds& S, uint32_t fp_pfx,
                                                        uint32_t o, uint32_t sh, uint32_t& s0, uint32_t& s1,
                                                        uint32_t& s2, uint32_t& s3, uint32_t& tot,
                                                        uint32_t* evw = nullptr) {
  const uint32_t w0 = my[o], w1 = my[o + 1], w2 = my[o + 2];
  unsigned long long win = ((((unsigned long long)w0 << 32) | w1) << sh) | (((unsigned long long)w2 << sh) >> 32);
  tot = 0;
  const uint32_t pfx = fsym(win, tot, S, fp_pfx);
  if (pfx < (uint32_t)P_RUN1) {
    const bool rgb = pfx == (uint32_t)P_RGB, lu = pfx == (uint32_t)P_LUMA, l2 = pfx == (uint32_t)P_LUMA2;
    const uint4 pp = S.pp[pfx];
    s0 = fsym(win, tot, S, pp.x);
    if constexpr (EV) *evw = (pfx << EV_PFX_SHIFT) | (s0 << ((pp.x >> 5) & 31u));
    if (rgb || lu || l2) {
      s1 = fsym(win, tot, S, pp.y);
      s2 = fsym(win, tot, S, pp.z);
      if constexpr (EV) *evw |= (s1 << ((pp.y >> 5) & 31u)) | (s2 << ((pp.z >> 5) & 31u));
      if (lu) {
        s3 = fsym(win, tot, S, pp.w);
        if constexpr (EV) *evw |= s3 << ((pp.w >> 5) & 31u);
      }
    }
  }
  return pfx;
}
// the same at a lane's own position (dec_sync_settle's walk; G: fast parameters), no per-symbol refill
__device__ __forceinline__ uint32_t pixel_event_fast(Lane& L, const uint32_t* my, const LutLds& S,
                                                     const StreamParams& G, uint32_t& s0, uint32_t& s1,
                                                     uint32_t& s2, uint32_t& s3) {
  uint32_t tot;
  const uint32_t pfx = pixel_event_fast_at(my, S, G.g[PFX_STREAM], (uint32_t)(L.pos >> 5) - L.ws,
                                           (uint32_t)L.pos & 31u, s0, s1, s2, s3, tot);
  L.pos += tot;
  return pfx;
}

// Event layout: the slices of a frame in groups of 64 (one parse wave); a
// group's events are interleaved in 16-byte quads, quad c of the group's slice
// l at words (c * 64 + l) * 4.  The first pass keeps every active lane at the
// same event index, so each of its 16-byte stores is one contiguous 1 KB per
// wave (a per-slice layout made every store touch 64 lines: +10 % parse time).
// Frames are padded to a multiple of 64 slices.
// (cap: a.ev_cap events per slice; the re-parses' head events, a.hev: the same layout, a.hev_cap)
__device__ __forceinline__ uint64_t ev_group(const DecArgs& a, uint32_t f, uint32_t j, uint32_t cap) {
  return ((uint64_t)f * ((a.max_chunks + 63u) & ~63u) + (j & ~63u)) * cap + (j & 63u) * 4u;
}
__device__ __forceinline__ uint32_t ev_word(uint32_t y) { return (y >> 2) * 256u + (y & 3u); }

// A slice's entry (nice_dec_state.hpp): the first slice starts at the data start.
__device__ __forceinline__ unsigned long long slice_entry(const DecArgs& a, uint64_t base, uint32_t j) {
  return j == 0 ? 0ull : a.entry[base + j];
}

// Who writes a slice's records once the parse is at its fixpoint (dec_heads,
// dec_emit and dec_place all decide it here):
//   SLICE_EMIT       dec_emit parses the whole slice: the final parse never met
//                    the first pass, or the first pass's events overflowed
//   SLICE_HEAD_EMIT  dec_emit parses the head up to the meeting checkpoint,
//                    dec_place writes the first pass's events from there
//   SLICE_PLACE      dec_place writes both: the head from the events the
//                    latest re-parse kept (none when the first pass itself
//                    started at the slice's final entry), then the first pass's
// A kept head stands only for a consistent slice (parsed last from its present
// entry) whose latest re-parse met the previous parse at `agree`, the latest
// meeting point of all passes: a re-parse that met earlier has overwritten the
// events between its meeting point and `agree`.
constexpr uint32_t SLICE_EMIT = 0, SLICE_HEAD_EMIT = 1, SLICE_PLACE = 2;
// hn: the head events dec_place walks (SLICE_PLACE), else 0.  (Every load is
// issued before the first is used: dec_place's short waves wait on them.)
__device__ __forceinline__ uint32_t slice_route(const DecArgs& a, uint64_t base, uint32_t j, uint32_t& ag,
                                                uint32_t& nvalid, uint32_t& hn) {
  const unsigned long long last = a.last[base + j];
  ag = a.agree[base + j];
  const uint32_t nev = a.ev_n[base + j];
  unsigned long long e = 0;
  uint32_t hev_n = EV_OVERFLOW, hev_ag = AGREE_NONE;
  if (a.hev) {
    e = slice_entry(a, base, j);
    hev_n = a.hev_n[base + j];
    hev_ag = a.hev_ag[base + j];
  }
  nvalid = last_nck(last);
  hn = 0;
  if (ag == AGREE_NONE || nev == EV_OVERFLOW || ag > nvalid) return SLICE_EMIT;
  if (ag == 0u) return SLICE_PLACE;
  if (!last_from(last, e) || hev_n == EV_OVERFLOW || hev_ag != ag) return SLICE_HEAD_EMIT;
  hn = hev_n;
  return SLICE_PLACE;
}

// (The event word of a parsed pixel -- ev_pack -- is nice_dec_event.hpp's.)

// ---------------------------------------------------------------------------
// Stages every parse kernel runs (dec_sync, dec_sync_settle, dec_strict_refill,
// dec_emit).
// ---------------------------------------------------------------------------
// A frame and a lane's view of it.  Two parts, in the order the kernels have
// always had: parse_frame before the kernel decides whether the block has work
// (block-uniform values); then the kernel loads the tables (load_lut, a
// barrier) and drops the waves without an item; then parse_lane: the stream
// parameters, the lane's ring, the stream pointer.  (Loading all of it up
// front cost dec_emit 11 VGPRs, and the table load inside parse_lane cost
// dec_sync 5 VGPRs and 45 vector instructions.)
struct ParseCtx {
  uint64_t len, D;          // the stream's bytes, its first data bit
  uint32_t nc;              // slices
  uint64_t base;            // the frame's first slice in the per-slice arrays
  StreamParams SP;
  uint32_t* wring;          // the wave's 64 rings
  const uint32_t* my;       // the lane's
  const uint8_t* p;         // the stream
  bool al16;
  unsigned long long hard;  // no parse goes on past this bit
};
__device__ __forceinline__ ParseCtx parse_frame(const DecArgs& a, uint32_t f) {
  ParseCtx C;
  C.len = a.stream_len[f];
  C.D = a.data_start[f];
  C.nc = n_chunks(C.len, C.D, a.chunk_bits);
  C.base = (uint64_t)f * a.max_chunks;
  return C;
}
// the block's lanes take items first .. first + blockDim.x - 1 of n: this wave has none
__device__ __forceinline__ bool wave_idle(uint32_t first, uint32_t n) { return first + (threadIdx.x >> 6) * 64u >= n; }
__device__ __forceinline__ void parse_lane(ParseCtx& C, const LutLds& S, uint32_t* ring, const DecArgs& a,
                                           uint32_t f) {
  const uint32_t wave = threadIdx.x >> 6;
  C.SP.load(S);
  C.wring = ring + wave * 64u * RING_STRIDE;
  C.my = C.wring + (threadIdx.x & 63u) * RING_STRIDE;
  C.p = dec_stream_ptr(a, f);
  C.al16 = (reinterpret_cast<uintptr_t>(C.p) & 15u) == 0;
  C.hard = C.len * 8 + 64;
}
// the frame's tables allow the fast parse (one lookup per symbol, events <= 64 bits)
__device__ __forceinline__ bool parse_fast(const DecArgs& a, uint32_t f) {
  return !a.parse_slow && reinterpret_cast<const DecTables*>(a.tables)[f].fast;
}
// A lane positioned at an entry, its ring empty (filled on the first step).
__device__ __forceinline__ Lane lane_at(const ParseCtx& C, unsigned long long e, uint32_t& dk) {
  Lane L;
  L.pos = C.D + ps_pos(e);
  L.rp = RING_W;
  L.ws = (uint32_t)(L.pos >> 5) - RING_W;   // (fast parse) empty as well
  dk = ps_dk(e);
  return L;
}

// The symbol-by-symbol parses' refill: the wave refills its rings when an
// active lane's has run out (or the lane forces it); then each active lane
// reads one pixel event (pixel_event, pixel_event_fast).  True when it refilled.
template <bool FAST = false>
__device__ __forceinline__ bool wave_refill(const ParseCtx& C, Lane& L, bool active, bool force = false) {
  if (!__any(active && (force || !(FAST ? lane_ok_fast(L) : lane_ok(L))))) return false;
  ring_fill<FAST>(C.wring, C.p, C.len, C.al16, L);
  return true;
}

// The fast parse in 32-bit positions (dec_sync's loop as RelCursor; dec_emit
// keeps the same few lines as locals, with rel_base and rel_fits): r =
// bits past B, the word holding the slice's first bit or, when the entry lies
// before the slice (the previous slice's parse stopped at px > N: speculative
// garbage), the entry's word.  The slice end, the stream end and the ring
// offsets are then 32-bit compares and adds instead of 64-bit ones.
__device__ __forceinline__ unsigned long long rel_base(bool active, unsigned long long pos, unsigned long long begin) {
  return (active && pos < begin ? pos : begin) & ~31ull;
}
// every lane of the wave within 2^30 bits of its B (else: the general parse)
__device__ __forceinline__ bool rel_fits(bool active, unsigned long long pos, unsigned long long B,
                                         unsigned long long end) {
  return __all(!active || (pos >= B && end - B < (1ull << 30)));
}
struct RelCursor {
  uint32_t fp_pfx;   // the prefix stream's fast parameter (the payload streams' come from S.pp;
                     // a converted copy of SP put SP in scratch for the general loop)
  uint32_t bwl;      // B's stream word
  uint32_t rlim;     // the lane stops at the first prefix at or past it: slice end or stream end
  uint32_t r;        // the lane's position
  uint32_t wsr = 0, rfill = 0;   // ring start word (relative); refill once r reaches rfill (ring empty: at once)
  __device__ __forceinline__ void init(const ParseCtx& C, unsigned long long B, unsigned long long pos,
                                       unsigned long long end, bool active) {
    fp_pfx = fast_param(C.SP.g[PFX_STREAM]);
    bwl = (uint32_t)(B >> 5);
    const uint32_t rhard = C.hard > B ? (uint32_t)min(C.hard - B, (unsigned long long)0xFFFFFFFFu) : 0u;
    rlim = active ? min((uint32_t)(end - B), rhard) : 0u;
    r = active ? (uint32_t)(pos - B) : 0u;
  }
  // (all 64 lanes) the next event's 3 words would pass the ring's end
  __device__ __forceinline__ void refill(const ParseCtx& C, bool active) {
    if (__any(active && r >= rfill)) {
      const uint32_t wsa = (bwl + (r >> 5)) & ~3u;
      ring_fill_ws(C.wring, C.p, C.len, C.al16, wsa);
      wsr = wsa - bwl;
      rfill = (wsr + RING_W - 2u) << 5;
    }
  }
  // one pixel event at r (pixel_event_fast_at), r past it
  template <bool EV = false>
  __device__ __forceinline__ uint32_t event(const ParseCtx& C, const LutLds& S, uint32_t& s0, uint32_t& s1,
                                            uint32_t& s2, uint32_t& s3, uint32_t* evw = nullptr) {
    uint32_t tot;
    const uint32_t pfx = pixel_event_fast_at<EV>(C.my, S, fp_pfx, (r >> 5) - wsr, r & 31u, s0, s1, s2, s3, tot, evw);
    r += tot;
    return pfx;
  }
};

}  // namespace nice
