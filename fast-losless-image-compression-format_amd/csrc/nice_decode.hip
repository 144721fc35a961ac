// nice_decode.hip -- MI355X (gfx950) decoder for the NICE2 bitstream.
//
// The reference decoder (code.rs:464-687) is one serial loop: a single
// context-switched Huffman stream (10 tables, grammar of code.rs:576-671) and a
// raster recurrence in which every pixel depends on its left neighbour (linear
// i-1, wrapping across rows) and on pixels up to 3W+3 back.  The GPU path splits
// it into:
//   dec_tables       header (code.rs:469-483), the 10 length tables
//                    (hfe.rs:173-190), canonical codes (hfe.rs:255-296) and a
//                    2-level lookup equivalent to the reference 2^max LUT.
//   dec_sync         chunk-parallel speculative parse: every CHUNK_BITS slice is
//                    decoded from a guessed entry state; exits become the next
//                    slice's entry (Jacobi iteration) until a fixpoint -- Huffman
//                    self-synchronisation makes this converge in a few passes.
//                    Re-parses stop at the first checkpoint where they agree
//                    with the previous parse; the sync pass also counts pixels.
//   dec_scan         exclusive scan of the pixel counts per frame.
//   dec_emit         one 32-bit record per coded pixel (mode + constants).
// The records go to the row kernels (nice_rows.hip: dec_reconstruct, dec_rows*),
// which rebuild the pixels row by row.
// This file keeps the kernels.  The parse machinery and the stages the four
// parse kernels share are nice_parse.hpp's; the packed words they exchange
// (slice entry, `last`, checkpoint) and the pixel arithmetic, nice_dec_state.hpp's;
// the event word and the records, nice_dec_event.hpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/nice.h"
#include "nice_bits.hpp"
#include "nice_dec_rec.hpp"
#include "nice_format.h"
#include "nice_kernels.h"
#include "nice_parse.hpp"

namespace nice {

// ---------------------------------------------------------------------------
// D0: tables. One block of 256 threads per frame.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dec_tables(DecArgs a) {
  __shared__ uint8_t lens[N_BINS];
  __shared__ uint8_t smax[N_STREAMS];
  __shared__ uint16_t order[N_BINS];
  __shared__ int bad;
  const uint32_t f = blockIdx.x;
  const uint64_t len = a.stream_len[f];
  DecTables* T = reinterpret_cast<DecTables*>(a.tables) + f;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  if (a.stream_off) {
    // packed batch: the stream must start on a granule and lie inside the
    // buffer -- checked before any byte of it is read
    const uint64_t o = a.stream_off[f];
    if ((o & 15u) || o > a.packed_bytes || len > a.packed_bytes - o) {
      if (threadIdx.x == 0) set_status(&a.status[f], NICE_E_ARG);
      return;
    }
  }
  const uint8_t* s = dec_stream_ptr(a, f);
  if (len < (uint64_t)FILE_HEADER_BYTES + (TABLE_HEADER_BITS + 7) / 8) {
    if (threadIdx.x == 0) set_status(&a.status[f], NICE_E_FORMAT);
    return;
  }
  // header: width/height must match the batch shape; channels byte 3 (reference
  // stride) or 4 (evident intent: RGBA with alpha not coded)
  const uint32_t w = ((uint32_t)s[4] << 24) | ((uint32_t)s[5] << 16) | ((uint32_t)s[6] << 8) | s[7];
  const uint32_t h = ((uint32_t)s[8] << 24) | ((uint32_t)s[9] << 16) | ((uint32_t)s[10] << 8) | s[11];
  const uint32_t ch = s[12];
  if (w != a.W || h != a.H) {
    if (threadIdx.x == 0) set_status(&a.status[f], NICE_E_ARG);
    return;
  }
  // the host sized the slice scratch from its copy of the lengths
  // (nice_decode_batch_dev_hl): a device length past that bound or the stream
  // stride fails the frame before any kernel indexes slices by it (packed
  // batches: the offset checks above take the stride's place)
  if ((!a.stream_off && len > a.stream_stride) ||
      n_chunks(len, FILE_HEADER_BYTES * 8 + TABLE_HEADER_BITS, a.chunk_bits) > a.max_chunks) {
    if (threadIdx.x == 0) set_status(&a.status[f], NICE_E_ARG);
    return;
  }
  if (ch != 3 && !(ch == 4 && !(a.flags & NICE_DEC_STRICT_REFERENCE))) {
    // code.rs:659 advances by 3 bytes while every other offset uses `channels`:
    // only channels == 3 decodes in the reference.
    if (threadIdx.x == 0) set_status(&a.status[f], NICE_E_UNSUPPORTED);
    return;
  }
#ifdef NICE_PROF_DTABLES
  long long tp[10];
  int tpn = 0;
#define DT_MARK() do { if (tpn < 10) tp[tpn++] = clock64(); } while (0)
#else
#define DT_MARK() do {} while (0)
#endif
  DT_MARK();
  // the file and table headers (770 bytes) staged in LDS as big-endian words
  // with one load per thread (the fields were ~12 dependent global reads per
  // thread: most of this kernel's time for a single frame)
  constexpr int HDR_WORDS = (FILE_HEADER_BYTES * 8 + TABLE_HEADER_BITS + 31) / 32 + 2;
  __shared__ uint32_t hw[HDR_WORDS];
  {
    const BitSrc src{s, len};
    for (int i = threadIdx.x; i < HDR_WORDS; i += 256) hw[i] = src.peek32((uint64_t)i * 32u);
  }
  __syncthreads();
  auto hpeek = [&](uint32_t pos) -> uint32_t {   // 32 bits at header bit pos, MSB first
    const uint32_t wi = pos >> 5, o = pos & 31u;
    return (uint32_t)((((unsigned long long)hw[wi] << 32 | hw[wi + 1]) << o) >> 32);
  };
  // Decoder side field widths are fixed: a 5-bit max (<= 31) always selects
  // 7-bit length fields (hfe.rs:177-178).
  for (int st = threadIdx.x; st < N_STREAMS; st += 256) {
    uint32_t pos = FILE_HEADER_BYTES * 8;
    for (int q = 0; q < st; ++q) pos += 5 + 7 * stream_size(q);
    smax[st] = (uint8_t)(hpeek(pos) >> 27);
  }
  for (int i = threadIdx.x; i < N_BINS; i += 256) {
    int st = 0;
    while (st + 1 < N_STREAMS && i >= stream_base(st + 1)) ++st;
    uint32_t pos = FILE_HEADER_BYTES * 8 + 5;
    for (int q = 0; q < st; ++q) pos += 5 + 7 * stream_size(q);
    lens[i] = (uint8_t)(hpeek(pos + 7u * (uint32_t)(i - stream_base(st))) >> 25);
  }
  __syncthreads();
  DT_MARK();
  const bool tolerant = (a.flags & NICE_DEC_TOLERANT_HEADER) && !(a.flags & NICE_DEC_STRICT_REFERENCE);
  if (tolerant) {
    // Spilled max fields (oracle tolerant_tables): a max above 31
    // keeps its low 5 bits in the field and adds max >> 5 into the p bits still
    // pending in the writer's u32 cache -- the low p bits of the previous
    // stream's last length, p = table-header bits written so far mod 8.  Undo it
    // from the last stream down; the table max becomes the longest decodable
    // (<= 31 bit) length.
    if (threadIdx.x == 0) {
      for (int st = N_STREAMS - 1; st >= 0; --st) {
        const int n = stream_size(st), b = stream_base(st);
        uint32_t mx = 0, dm = 0;
        for (int i = 0; i < n; ++i) {
          const uint32_t l = lens[b + i];
          mx = max(mx, l);
          if (l <= 31) dm = max(dm, l);
        }
        if ((mx & 31u) != smax[st] || mx > 127 || dm == 0) bad = 1;
        if (mx >= 32 && st > 0) {
          uint32_t bits = 0;
          for (int q = 0; q < st; ++q) bits += 5u + 7u * (uint32_t)stream_size(q);
          const uint32_t pm = (1u << (bits & 7u)) - 1u;
          uint8_t& last = lens[stream_base(st - 1) + stream_size(st - 1) - 1];
          last = (uint8_t)((last & ~pm) | ((last - (mx >> 5)) & pm));
        }
        smax[st] = (uint8_t)dm;
      }
    }
    __syncthreads();
    // every stream a complete prefix code over all its lengths (Kraft sum 1)
    if (threadIdx.x < N_STREAMS) {
      const int st = threadIdx.x, n = stream_size(st), b = stream_base(st);
      uint32_t mx = 0;
      bool ok = true;
      for (int i = 0; i < n; ++i) { mx = max(mx, (uint32_t)lens[b + i]); ok = ok && lens[b + i] >= 1; }
      unsigned __int128 kraft = 0;
      for (int i = 0; i < n && ok; ++i) kraft += (unsigned __int128)1 << (mx - lens[b + i]);
      if (!ok || kraft != ((unsigned __int128)1 << mx)) atomicOr(&bad, 1);
    }
  } else {
    // validity: every length in [1, max], max attained, Kraft sum == 1 -- every
    // symbol at once, per-stream sums by LDS atomics (a lane per stream looping
    // over its symbols took ~0.13 ms of a single frame's decode)
    __shared__ unsigned long long vkraft[N_STREAMS];
    __shared__ uint32_t vseen[N_STREAMS];
    if (threadIdx.x < N_STREAMS) { vkraft[threadIdx.x] = 0; vseen[threadIdx.x] = 0; }
    __syncthreads();
    for (int i = threadIdx.x; i < N_BINS; i += 256) {
      int st = 0;
#pragma unroll
      for (int q = 1; q < N_STREAMS; ++q) st += i >= stream_base(q) ? 1 : 0;
      const uint32_t mx = smax[st], l = lens[i];
      if (l < 1 || l > mx || mx > 31) atomicOr(&bad, 1);
      else {
        atomicAdd(&vkraft[st], 1ull << (mx - l));
        atomicMax(&vseen[st], l);
      }
    }
    __syncthreads();
    if (threadIdx.x < N_STREAMS) {
      const int st = threadIdx.x;
      const uint32_t mx = smax[st];
      if (mx < 1 || vseen[st] != mx || vkraft[st] != (1ull << mx)) atomicOr(&bad, 1);
      // strict: tables of 26..31 bits can make the reference's refill loop wrap
      // its u8 bit offset (bitreader.rs:88-97); dec_strict_refill finds the reads
      // where it does
    }
  }
  __syncthreads();
  if (bad) {
    if (threadIdx.x == 0) set_status(&a.status[f], NICE_E_UNSUPPORTED);
    return;
  }
  DT_MARK();
  // canonical order per stream: rank by (len desc, symbol desc)
  for (int st = 0; st < N_STREAMS; ++st) {
    const int n = stream_size(st), b = stream_base(st);
    for (int i = threadIdx.x; i < n; i += 256) {
      const uint8_t li = lens[b + i];
      int rank = 0;
#pragma unroll 8
      for (int j = 0; j < n; ++j) {   // independent reads: unrolled, batched
        const uint8_t lj = lens[b + j];
        rank += (lj > li) || (lj == li && j > i);
      }
      order[b + rank] = (uint16_t)i;
    }
  }
  __syncthreads();
  DT_MARK();
  __shared__ uint8_t lbits[N_STREAMS];
  __shared__ uint16_t loff[N_STREAMS];
  if (threadIdx.x == 0) {
    // first-level widths: the full max length where possible, shrinking the
    // widest tables until all ten fit the budget (long codes take the search)
    uint32_t tot = 0;
    for (int st = 0; st < N_STREAMS; ++st) {
      lbits[st] = (uint8_t)min((uint32_t)smax[st], (uint32_t)DEC_LUT_MAX_BITS);
      tot += 1u << lbits[st];
    }
    while (tot > (uint32_t)DEC_LUT_BUDGET) {
      int w = 0;
      for (int st = 1; st < N_STREAMS; ++st) if (lbits[st] > lbits[w]) w = st;
      tot -= 1u << (lbits[w] - 1);
      lbits[w] -= 1;
    }
    uint32_t o = 0;
    for (int st = 0; st < N_STREAMS; ++st) { loff[st] = (uint16_t)o; o += 1u << lbits[st]; }
  }
  __syncthreads();
  DT_MARK();
  // canonical codes (hfe.rs:271-290): one lane per stream, serial in LDS; the
  // lengths in rank order first (all threads), so the serial loop reads one
  // independent word per symbol instead of a dependent order -> length chain
  __shared__ uint32_t clo[N_BINS];
  __shared__ uint8_t clen[N_BINS];
  for (int i = threadIdx.x; i < N_BINS; i += 256) {
    int st = 0;
#pragma unroll
    for (int q = 1; q < N_STREAMS; ++q) st += i >= stream_base(q) ? 1 : 0;
    clen[i] = lens[stream_base(st) + order[i]];
  }
  __syncthreads();
  if (threadIdx.x < N_STREAMS) {
    const int st = threadIdx.x;
    const int n = stream_size(st), b = stream_base(st);
    const uint32_t mx = smax[st];
    T->max_aob[st] = (uint8_t)mx;
    T->lut_bits[st] = lbits[st];
    T->lut_off[st] = loff[st];
    // usize wrapping (shift amounts masked to 6 bits); in tolerant mode lengths
    // above 31 (zero-count symbols) get no decode entry (lo above every 31-bit
    // window value) and the decodable codes must fit their lengths and not
    // overlap
    unsigned long long cur = 0;
    uint32_t prev = 0;
    uint64_t prev_lo = ~0ull;
    bool ok = true;
#pragma unroll 4
    for (int k = 0; k < n; ++k) {
      const uint32_t l = clen[b + k];
      if (l < prev) cur >>= (prev - l) & 63u;
      if (prev > 0) cur += 1;
      const unsigned long long code64 = (1ull << (l & 63u)) - cur - 1ull;
      prev = l;
      if (l > mx) { clo[b + k] = 0xFFFFFFFFu; continue; }
      const uint64_t lo = (uint64_t)(uint32_t)code64 << (mx - l);
      if ((code64 >> l) != 0 || (prev_lo != ~0ull && lo + (1ull << (mx - l)) > prev_lo)) ok = false;
      prev_lo = lo;
      clo[b + k] = (uint32_t)lo;
    }
    if (!ok) atomicOr(&bad, 1);
  }
  __syncthreads();
  if (bad) {
    if (threadIdx.x == 0) set_status(&a.status[f], NICE_E_UNSUPPORTED);
    return;
  }
  DT_MARK();
  for (int i = threadIdx.x; i < N_BINS; i += 256) {
    T->lo[i] = clo[i];
    T->sym[i] = order[i];
    T->len[i] = clen[i];
  }
  // first-level entries, all streams in parallel: entry e of stream st is the
  // window value x = e << (max - width); the code covering it is the first in
  // canonical order (lower bounds descending) with lo <= x -- a complete,
  // non-overlapping code (checked above) covers every x exactly once.  A code
  // longer than the width leaves the long-code marker 0.
  DT_MARK();
  const uint32_t n_lut = (uint32_t)loff[N_STREAMS - 1] + (1u << lbits[N_STREAMS - 1]);
  __shared__ int lut_hole;
  if (threadIdx.x == 0) lut_hole = 0;
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < n_lut; e += 256) {
    int st = 0;
#pragma unroll
    for (int q = 1; q < N_STREAMS; ++q) st += e >= loff[q] ? 1 : 0;   // independent reads, no search loop
    const uint32_t lb = lbits[st], mx = smax[st];
    const uint32_t x = (e - loff[st]) << (mx - lb);
    int lo = stream_base(st), hi = lo + stream_size(st) - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (clo[mid] <= x) hi = mid;
      else lo = mid + 1;
    }
    const uint32_t l = clen[lo];
    T->lut[e] = l <= lb ? (uint16_t)(((uint32_t)order[lo] << 5) | l) : (uint16_t)0;
    if (l > lb || l == 0) lut_hole = 1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // longest pixel event: the prefix plus the longest payload sequence (code.rs:576-644)
    const uint32_t m_pay = max(max((uint32_t)smax[S_BACK_REF], 3u * smax[S_RGB]),
                               max((uint32_t)smax[S_LUMA_REF] + smax[S_LUMA_BASE] + 2u * smax[S_LUMA_OTHER],
                                   max((uint32_t)smax[S_SMALL_DIFF],
                                       (uint32_t)smax[S_LUMA2_BASE] + smax[S_LUMA2_R] + smax[S_LUMA2_B])));
    T->fast = (!lut_hole && smax[S_PREFIX] + m_pay <= 64u) ? 1u : 0u;
    a.data_start[f] = FILE_HEADER_BYTES * 8 + TABLE_HEADER_BITS;
  }
#ifdef NICE_PROF_DTABLES
  DT_MARK();
  if (threadIdx.x == 0 && f == 0)
    printf("dec_tables cycles: stage+lens %lld valid %lld rank %lld widths %lld canon %lld copy %lld lut %lld (n=%d)\n",
           tp[1] - tp[0], tp[2] - tp[1], tp[3] - tp[2], tp[4] - tp[3], tp[5] - tp[4], tp[6] - tp[5], tp[7] - tp[6], tpn);
#endif
}

// Initial entry guesses: every slice starts at its first bit, at a prefix.
__global__ __launch_bounds__(256) void dec_init_entries(DecArgs a) {
  const uint32_t f = blockIdx.y;
  for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < a.max_chunks; j += gridDim.x * 256) {
    const uint64_t i = (uint64_t)f * a.max_chunks + j;
    a.entry[i] = ps_pack((unsigned long long)j * a.chunk_bits, 0);
    a.last[i] = LAST_NEVER;
  }
}


// ---------------------------------------------------------------------------
// D1: sync iteration (Jacobi, in place).  Each lane parses its slice from the
// current entry guess and writes the exit as the next slice's entry.  Lanes
// whose entry did not change since their last parse do nothing.  A re-parse
// compares its state with the previous parse at the first prefix after every
// CK_BITS; once they agree the rest of the slice is unchanged (Huffman
// self-synchronisation), so the lane stops and only patches its pixel count.
// ---------------------------------------------------------------------------
// `prev`: the previous iteration's change flag -- when it is 0 the entries are
// at the fixpoint already and this launch does nothing (the host queues several
// iterations without waiting for each).
// `fchanged` (optional): per-frame change flags, for dec_sync_settle.
__global__ __launch_bounds__(DEC_PARSE_THREADS) PARSE_ATTR void dec_sync(DecArgs a, uint32_t* changed, const uint32_t* prev,
                                                              uint32_t* fchanged) {
  __shared__ LutLds S;
  __shared__ __attribute__((aligned(16))) uint32_t ring[DEC_PARSE_THREADS * RING_STRIDE];
  if (prev && *prev == 0) return;
  const uint32_t f = blockIdx.x / a.chunk_blocks;
  const uint32_t jb = blockIdx.x % a.chunk_blocks;
  if (a.status[f] != 0) return;
  ParseCtx C = parse_frame(a, f);
  const uint64_t D = C.D, base = C.base;
  const uint32_t nc = C.nc;
  if (jb * DEC_PARSE_THREADS >= nc) return;
  const uint32_t j = jb * DEC_PARSE_THREADS + threadIdx.x;
  unsigned long long e = 0, last = LAST_NEVER;
  if (j < nc) {
    e = slice_entry(a, base, j);
    last = a.last[base + j];
  }
  const bool need = j < nc && (last_never(last) || !last_from(last, e));
  if (!__syncthreads_or(need)) return;
  load_lut(S, reinterpret_cast<const DecTables*>(a.tables) + f);
  __syncthreads();
  if (wave_idle(jb * DEC_PARSE_THREADS, nc)) return;
  parse_lane(C, S, ring, a, f);
  const bool check = !last_never(last);
  const uint32_t nvalid_old = last_nck(last);
  const unsigned long long begin = D + (unsigned long long)j * a.chunk_bits;
  const unsigned long long end = begin + a.chunk_bits;
  const uint32_t N = a.W * a.H;
  unsigned long long* ck = a.ck + (uint64_t)f * a.n_ck * a.max_chunks + j;
  // first pass: keep the pixel events (16-byte stores of 4)
  const bool keep = a.ev != nullptr && !check;
  // (one pointer: a lane keeps the first pass's events or a re-parse's head, never both)
  uint32_t* evp = check ? a.hev + ev_group(a, f, j, a.hev_cap) : a.ev + ev_group(a, f, j, a.ev_cap);
  uint32_t* evck = a.ev_ck + (uint64_t)f * a.n_ck * a.max_chunks + j;
  // re-parses: keep the head's events, from the entry to the checkpoint where
  // the parse meets the previous one (ne counts them, as the first pass's)
  const bool hkeep = a.hev != nullptr && check && need;
  bool hkept = false;   // (wave-uniform) the loop this wave took kept them
  uint32_t ne = 0, ev0 = 0, ev1 = 0, ev2 = 0;
  uint32_t dk;
  Lane L = lane_at(C, e, dk);
  uint32_t px = 0, k = 0;
  unsigned long long next_ck = begin + a.ck_bits;
  unsigned long long ck_old = (check && nvalid_old > 0) ? ck[0] : ~0ull;
  bool active = need, synced = false;
  // diagnostics (builds with -DNICE_SYNC_CYCLES and NICE_DEC_STATS=1, first
  // pass): wave cycles, refill cycles / count, iterations.  Compiled out by
  // default: the checks alone cost ~2 % of the kernel.
  unsigned long long tw0 = 0, tfill = 0, nfill = 0, nit = 0, nact = 0;
#ifdef NICE_SYNC_CYCLES
  const bool tstat = a.stats != nullptr && !check;
#else
  constexpr bool tstat = false;
#endif
  if (tstat) tw0 = __builtin_amdgcn_s_memtime();
  // At the first prefix at or past a checkpoint's bit (pos: bits into the
  // slice): a re-parse that agrees with the previous parse stops here, else the
  // checkpoint is written: true, and the caller moves on to the next one.
  auto checkpoint = [&](uint32_t pos) __attribute__((always_inline)) -> bool {
    const uint32_t cur = ck_key(pos, dk);
    if (check && k < nvalid_old && ck_key_of(ck_old) == cur) {
      synced = true;
      active = false;
      return false;
    }
    ck[(uint64_t)k * a.max_chunks] = ck_pack(cur, px);
    if (keep) evck[(uint64_t)k * a.max_chunks] = ne;
    ++k;
    ck_old = (check && k < nvalid_old) ? ck[(uint64_t)k * a.max_chunks] : ~0ull;
    return true;
  };
  // Fast parse in 32-bit positions (RelCursor; the checkpoints too): the loop
  // is unrolled four times so a kept event goes straight into its slot of the
  // 16-byte quad (every active lane of the first pass is at the same event
  // index) instead of through a shift register.  A wave with a lane more than
  // 2^30 bits away takes the general symbol-by-symbol parse, which reads any
  // tables.
  const bool fast = parse_fast(a, f);
  const unsigned long long B = rel_base(active, L.pos, begin);
  if (fast && rel_fits(active, L.pos, B, end)) {
    RelCursor R;
    R.init(C, B, L.pos, end, active);
    const uint32_t b31 = (uint32_t)(begin - B);   // the slice's first bit
    uint32_t nck = b31 + a.ck_bits;   // next checkpoint (relative)
    uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;   // the current quad of kept events
    // keep_tag: 0 keeps nothing, 1 the first pass (events into ev), 2 a re-parse
    // (head events into hev)
    auto step = [&](auto slot_tag, auto keep_tag) -> bool {
      constexpr int SLOT = decltype(slot_tag)::value;
      constexpr bool KEEP = decltype(keep_tag)::value == 1;
      constexpr bool KEPT = decltype(keep_tag)::value != 0;
      if (active && (R.r >= R.rlim || px > N)) active = false;
      if (active && R.r >= nck && checkpoint(R.r - b31)) nck = k < a.n_ck ? nck + a.ck_bits : 0xFFFFFFFFu;
      // (the passes that keep events test for the wave's end once per quad: a
      // step after every lane stopped only evaluates masked conditions)
      if ((!KEPT || SLOT == 0) && !__any(active)) return false;
      R.refill(C, active);
      if (active) {
        uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, evw = 0;
        const uint32_t pfx = R.event<KEPT>(C, S, s0, s1, s2, s3, &evw);
        const uint32_t c = pixel_count(pfx, dk);
        px = sat_add(px, c);
        // (every re-parsing lane of the wave starts at event 0 in the same step, as the first pass's)
        if (KEPT && (KEEP ? keep : hkeep)) {
          const uint32_t ev = pfx < (uint32_t)P_RUN1 ? evw : EV_RUN | min(c, EV_RUN - 1u);
          if constexpr (SLOT == 0) q0 = ev;
          if constexpr (SLOT == 1) q1 = ev;
          if constexpr (SLOT == 2) q2 = ev;
          if constexpr (SLOT == 3) {
            q3 = ev;
            if (ne < (KEEP ? a.ev_cap : a.hev_cap))
              *reinterpret_cast<uint4*>(evp + ev_word(ne - 3u)) = make_uint4(q0, q1, q2, q3);
          }
          ++ne;
        }
      }
      return true;
    };
    auto quads = [&](auto keep_tag) __attribute__((always_inline)) {   // unrolled by the quad
      for (;;) {
        if (!step(std::integral_constant<int, 0>{}, keep_tag)) break;
        if (!step(std::integral_constant<int, 1>{}, keep_tag)) break;
        if (!step(std::integral_constant<int, 2>{}, keep_tag)) break;
        if (!step(std::integral_constant<int, 3>{}, keep_tag)) break;
      }
    };
    if (__any(keep && active)) {   // the first pass
      quads(std::integral_constant<int, 1>{});
    } else if (__any(hkeep && active)) {   // a re-parse keeping its head: the same way
      hkept = true;
      quads(std::integral_constant<int, 2>{});
    } else {   // a re-parse that keeps nothing (a smaller loop: these launches are short)
      while (step(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{})) {
      }
    }
    L.pos = B + R.r;
    // the tail below stores the last (ne & 3) events from ev0..ev2 (newest last)
    const uint32_t sl = ne & 3u;
    ev0 = q0;
    ev1 = sl == 3u ? q1 : q0;
    ev2 = sl == 3u ? q2 : sl == 2u ? q1 : q0;
  } else {   // (any tables; the general parse)
    for (;;) {
      // at a prefix position: slice end, checkpoint, or one more pixel event
      if (active && (L.pos >= end || L.pos >= C.hard || px > N)) active = false;
      if (active && L.pos >= next_ck && checkpoint((uint32_t)(L.pos - begin)))
        next_ck = k < a.n_ck ? next_ck + a.ck_bits : ~0ull;
      if (!__any(active)) break;
      const unsigned long long tf = tstat ? __builtin_amdgcn_s_memtime() : 0;
      if (wave_refill(C, L, active) && tstat) { tfill += __builtin_amdgcn_s_memtime() - tf; ++nfill; }
      if (tstat) { ++nit; nact += active ? 1u : 0u; }
      if (active) {
        uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        const uint32_t pfx = pixel_event(L, C.my, S, C.SP, s0, s1, s2, s3);
        const uint32_t c = pixel_count(pfx, dk);
        px = sat_add(px, c);
        if (keep || hkeep) {
          const uint32_t ev = pfx < (uint32_t)P_RUN1 ? ev_pack(pfx, s0, s1, s2, s3) : EV_RUN | min(c, EV_RUN - 1u);
          // the last three events in a shift register (ev2 the newest)
          if (ne < (keep ? a.ev_cap : a.hev_cap) && (ne & 3u) == 3u)
            *reinterpret_cast<uint4*>(evp + ev_word(ne - 3u)) = make_uint4(ev0, ev1, ev2, ev);
          ev0 = ev1;
          ev1 = ev2;
          ev2 = ev;
          ++ne;
        }
      }
    }
    hkept = true;
  }
  if (tstat) {
    const unsigned long long tw = __builtin_amdgcn_s_memtime() - tw0;
    if ((threadIdx.x & 63u) == 0) {
      atomicAdd(&a.stats[56], tw); atomicAdd(&a.stats[57], tfill); atomicAdd(&a.stats[58], nfill);
      atomicAdd(&a.stats[59], nit); atomicAdd(&a.stats[61], 1ull);
    }
    atomicAdd(&a.stats[60], nact);
  }
  if (!need) return;
  // the last (ne & 3) kept events are the newest of ev0..ev2
  auto store_tail = [&](uint32_t* t) {
    const uint32_t slot = ne & 3u;
    if (slot == 3u) { t[0] = ev0; t[1] = ev1; t[2] = ev2; }
    if (slot == 2u) { t[0] = ev1; t[1] = ev2; }
    if (slot == 1u) t[0] = ev2;
  };
  if (keep) {
    if (ne <= a.ev_cap) store_tail(evp + ev_word(ne & ~3u));
    a.ev_n[base + j] = ne <= a.ev_cap ? ne : EV_OVERFLOW;
    a.agree[base + j] = 0;
  } else if (a.ev) {
    // the final parse equals the first pass from the latest meeting point on
    const uint32_t ag = synced ? k + 1u : AGREE_NONE;
    a.agree[base + j] = max(a.agree[base + j], ag);
    if (a.hev) {
      // the head stands when this parse met the previous one within hev_cap
      // events; a later re-parse of the slice overwrites it
      const bool ok = synced && hkept && ne <= a.hev_cap;
      if (ok) store_tail(evp + ev_word(ne & ~3u));
      a.hev_n[base + j] = ok ? ne : EV_OVERFLOW;
      a.hev_ag[base + j] = ag;
    }
  }
  if (a.stats && check) {   // diagnostics: where re-parses met the previous parse (16: never)
    atomicAdd(&a.stats[32 + (synced ? min(k, 15u) : 16u)], 1ull);
  }
  if (synced) {
    // from checkpoint k on this parse equals the previous one, shifted by delta pixels
    const uint32_t delta = px - ck_px(ck_old);
    a.chunk_px[base + j] = a.chunk_px[base + j] + (uint64_t)(int64_t)(int32_t)delta;
    for (uint32_t kk = k; kk < nvalid_old; ++kk) {
      unsigned long long& c = ck[(uint64_t)kk * a.max_chunks];
      c = ck_add_px(c, delta);
    }
    a.last[base + j] = last_pack(e, nvalid_old);
    return;
  }
  a.chunk_px[base + j] = px;
  a.last[base + j] = last_pack(e, k);
  if (j + 1 < nc) {
    const unsigned long long x = ps_pack(L.pos - D, dk);
    if (a.entry[base + j + 1] != x) {
      a.entry[base + j + 1] = x;
      atomicOr(changed, 1u);
      if (fchanged) fchanged[f] = 1u;
    }
  }
}

// ---------------------------------------------------------------------------
// D1b: the fixpoint on the device, for frames whose entries still changed in the
// last queued Jacobi iteration (fchanged).  The exact entries are the serial
// chain E_0 = 0, E_{j+1} = exit(j, E_j) (code.rs:573-684 is one parse); what
// the Jacobi iterations left is used as far as it is provably on that chain:
//  * slice j is consistent when it was last parsed from its current entry
//    (last[j] == entry[j]): then entry[j+1] is exit(j, entry[j]);
//  * so a walk that arrives at slice j with the exact entry x == entry[j] of a
//    consistent slice continues at entry[j+1] without parsing, and only the
//    slices whose entry or parse is stale are parsed.
// The frame's slices are cut into contiguous ranges, one per lane of the
// block (512 lanes).  Round 0: every lane walks its range from the entry its
// first slice holds, skipping consistent slices, parsing the others and
// writing their exits as the next entries; the first range starts exact
// (E_0 = 0).  A round leaves each range internally consistent.  Then a lane
// whose start differs from its left neighbour's exit walks again from that
// exit, parsing only until it meets an entry it already holds (from there its
// range is consistent, so its exit stands); rounds repeat until no start
// changes.  Range r is exact once ranges 0..r-1 are, so this terminates; with
// self-synchronisation within a range it ends after round 1, and a stream
// that never re-synchronises costs one serial parse of its dirty slices, as
// the reference's own decode does.  (Round 5's settle had one lane walk every
// slice from slice 0: 3.3 s for a 4K frame that missed the fixpoint by one
// queued iteration.)  A dec_sync launch after this one (prev = *settled)
// re-parses the slices whose entries moved, bringing their pixel counts,
// checkpoints and meeting points up to date.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(SETTLE_THREADS) void dec_sync_settle(DecArgs a, const uint32_t* last_changed,
                                                                  const uint32_t* fchanged, uint32_t* settled) {
  __shared__ LutLds S;
  __shared__ __attribute__((aligned(16))) uint32_t ring[SETTLE_THREADS * RING_STRIDE];
  __shared__ unsigned long long xs[SETTLE_THREADS];   // each range's exit in the current round
  const uint32_t f = blockIdx.x;
  if (*last_changed == 0 || fchanged[f] == 0 || a.status[f] != 0) return;   // block-uniform
  ParseCtx C = parse_frame(a, f);
  const uint64_t D = C.D, base = C.base;
  const uint32_t nc = min(C.nc, a.max_chunks);
  if (nc < 2) return;
  load_lut(S, reinterpret_cast<const DecTables*>(a.tables) + f);
  __syncthreads();
  parse_lane(C, S, ring, a, f);   // (every wave stays: the rounds' barriers)
  const uint32_t t = threadIdx.x;
  const uint32_t N = a.W * a.H;
  const uint32_t per = (nc + SETTLE_THREADS - 1) / SETTLE_THREADS;
  const uint32_t lo = min(t * per, nc), hi = min(lo + per, nc);   // nonempty ranges: lanes 0..k, contiguous
  unsigned long long start = slice_entry(a, base, lo);
  unsigned long long xprev = 0;   // the lane's exit of the previous round
  bool walk = lo < hi;
  const bool fast = parse_fast(a, f);
  for (uint32_t round = 0;; ++round) {
    // ---- one round: the lanes with `walk` parse their range from `start`
    uint32_t dk;
    Lane L = lane_at(C, 0ull, dk);
    uint32_t j = lo, px = 0;
    unsigned long long end = 0, xout = xprev;
    bool refill = true;
    // position the lane at slice j with entry x, after the slices it may skip;
    // false once the walk is done (xout set)
    auto advance = [&](unsigned long long x) -> bool {
      for (;;) {
        if (j >= hi) { xout = x; return false; }
        const unsigned long long cur = slice_entry(a, base, j);
        if (round == 0) {
          const unsigned long long lj = a.last[base + j];
          if (x == cur && !last_never(lj) && last_from(lj, cur)) {   // consistent: its exit is the next entry
            x = j + 1 < nc ? a.entry[base + j + 1] : 0ull;
            ++j;
            continue;
          }
        } else if (j > lo && x == cur) {   // the rest of the range is consistent from here
          xout = xprev;
          return false;
        }
        if (j > lo) a.entry[base + j] = x;
        L.pos = D + ps_pos(x);
        dk = ps_dk(x);
        px = 0;
        end = D + (unsigned long long)(j + 1) * a.chunk_bits;
        refill = true;
        return true;
      }
    };
    bool active = walk && advance(start);
    auto parse = [&](auto fast_tag) {
      constexpr bool FAST = decltype(fast_tag)::value;
      StreamParams G = C.SP;
      if constexpr (FAST) {
#pragma unroll
        for (int i = 0; i < N_STREAMS; ++i) G.g[i] = fast_param(G.g[i]);
      }
      for (;;) {
        // at a prefix position: the slice's end (same stop rule as dec_sync), or one more pixel event
        if (active && (L.pos >= end || L.pos >= C.hard || px > N)) {
          ++j;
          active = advance(ps_pack(L.pos - D, dk));
        }
        if (!__any(active)) break;
        if (wave_refill<FAST>(C, L, active, refill)) refill = false;
        if (active) {
          uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
          const uint32_t pfx = FAST ? pixel_event_fast(L, C.my, S, G, s0, s1, s2, s3)
                                    : pixel_event(L, C.my, S, G, s0, s1, s2, s3);
          px = sat_add(px, pixel_count(pfx, dk));
        }
      }
    };
    if (fast) parse(std::true_type{});
    else parse(std::false_type{});
    xs[t] = xout;
    __syncthreads();
    // ---- a range whose start is not its left neighbour's exit walks again
    const unsigned long long want = (t == 0 || lo >= hi) ? start : xs[t - 1];
    xprev = xout;
    walk = want != start;
    if (walk) {
      start = want;
      a.entry[base + lo] = want;   // lane t - 1 reads it only in round 0
    }
    if (!__syncthreads_or(walk)) break;
  }
  if (t == 0) *settled = 1u;
}

// ---------------------------------------------------------------------------
// D3: exclusive scan of chunk pixel counts, one 1024-thread block per frame.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void dec_scan(DecArgs a) {
  __shared__ unsigned long long part[1024];
  const uint32_t f = blockIdx.x;
  if (a.status[f] != 0) return;
  if (a.unsettled && a.unsettled[f]) {   // the parse is not at its fixpoint: fail, never decode from it
    if (threadIdx.x == 0) set_status(&a.status[f], NICE_E_HIP);
    return;
  }
  const uint32_t nc = n_chunks(a.stream_len[f], a.data_start[f], a.chunk_bits);
  const uint64_t base = (uint64_t)f * a.max_chunks;
  const uint32_t per = (nc + 1023) / 1024;
  const uint32_t c0 = threadIdx.x * per, c1 = min(c0 + per, nc);
  // a thread's range in batches of 8 independent loads (one at a time, a
  // single frame's ~85 chunks per thread were ~85 dependent round trips)
  constexpr uint32_t B = 8;
  unsigned long long sum = 0;
  for (uint32_t j0 = c0; j0 < c1; j0 += B) {
    unsigned long long v[B];
#pragma unroll
    for (uint32_t q = 0; q < B; ++q) v[q] = j0 + q < c1 ? a.chunk_px[base + j0 + q] : 0ull;
#pragma unroll
    for (uint32_t q = 0; q < B; ++q) sum = (sum + v[q] < sum) ? ~0ull : sum + v[q];   // saturate (garbage past the image end)
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    unsigned long long v = part[threadIdx.x];
    if ((int)threadIdx.x >= d) {
      const unsigned long long u = part[threadIdx.x - d];
      v = (v + u < v) ? ~0ull : v + u;
    }
    __syncthreads();
    part[threadIdx.x] = v;
    __syncthreads();
  }
  unsigned long long run = threadIdx.x ? part[threadIdx.x - 1] : 0ull;
  for (uint32_t j0 = c0; j0 < c1; j0 += B) {
    unsigned long long v[B];
#pragma unroll
    for (uint32_t q = 0; q < B; ++q) v[q] = j0 + q < c1 ? a.chunk_px[base + j0 + q] : 0ull;
#pragma unroll
    for (uint32_t q = 0; q < B; ++q) {
      if (j0 + q < c1) a.chunk_start[base + j0 + q] = run;
      run = (run + v[q] < run) ? ~0ull : run + v[q];
    }
  }
  if (threadIdx.x == 1023) {
    // total must cover the image
    if (part[1023] < (unsigned long long)a.W * a.H) set_status(&a.status[f], NICE_E_FORMAT);
  }
}

// ---------------------------------------------------------------------------
// D3b (strict mode only): the reference's refill wrap (bitreader.rs:85-98).
// read_24bits_noclear(M) refills while its u8 bit offset exceeds 32 - M,
// subtracting 8 each time; the offset's residue mod 8 is the read position's
// (offset = P + 32 - 8 * bytes read), so the loop runs through the value P & 7
// and, when that is above 32 - M, subtracts 8 from it: the u8 wraps and the
// loop never ends.  A read therefore hangs the reference iff it refills at all
// -- P + M > 8 * bytes read so far -- and (P & 7) + M > 32 (only M >= 26).
// Bytes read are a running maximum of ceil((P_k + M_k) / 8) over the reads
// (M = the stream's max length, hfe.rs:209), starting at the 770 header bytes.
// The reads that end the decode: every event while pixels < N, then one more
// prefix (plus the zero digits of a run that reached N, which the reference's
// run loop keeps reading, code.rs:665-671).  One lane per slice re-parses the
// converged slice j - 1 (for its reads' running maximum; slices are >= 1024
// bits and only the last 31 bits of reads matter) and then checks slice j.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(DEC_PARSE_THREADS) void dec_strict_refill(DecArgs a) {
  __shared__ LutLds S;
  __shared__ __attribute__((aligned(16))) uint32_t ring[DEC_PARSE_THREADS * RING_STRIDE];
  const uint32_t f = blockIdx.x / a.chunk_blocks;
  const uint32_t jb = blockIdx.x % a.chunk_blocks;
  if (a.status[f] != 0) return;
  const DecTables* T = reinterpret_cast<const DecTables*>(a.tables) + f;
  uint32_t mx = 0;
#pragma unroll
  for (int st = 0; st < N_STREAMS; ++st) mx = max(mx, (uint32_t)T->max_aob[st]);
  if (mx <= 25u) return;   // (P & 7) + M <= 32 for every read
  ParseCtx C = parse_frame(a, f);
  const uint64_t D = C.D, base = C.base;
  const uint32_t nc = C.nc;
  if (jb * DEC_PARSE_THREADS >= nc) return;
  load_lut(S, T);
  __syncthreads();
  if (wave_idle(jb * DEC_PARSE_THREADS, nc)) return;
  parse_lane(C, S, ring, a, f);
  const StreamParams SP = C.SP;  // a copy of its own: rd indexes it dynamically (the kernel's 48 bytes of scratch)
  const uint32_t j = jb * DEC_PARSE_THREADS + threadIdx.x;
  const uint32_t j0 = j > 0 ? j - 1u : 0u;
  const unsigned long long N = (unsigned long long)a.W * a.H;
  const unsigned long long begin = D + (unsigned long long)j * a.chunk_bits;
  const unsigned long long end = begin + a.chunk_bits;
  bool active = j < nc;
  unsigned long long e = 0, q = 0;
  if (active) {
    e = slice_entry(a, base, j0);
    q = a.chunk_start[base + j0];
  }
  uint32_t dk;
  Lane L = lane_at(C, e, dk);
  bool closed = q == N;
  unsigned long long nb8 = D;   // 8 x bytes the reference has read (D = 770 bytes)
  bool hang = false;
  for (;;) {
    if (active && (L.pos >= end || L.pos >= C.hard || q > N)) active = false;
    if (!__any(active)) break;
    (void)wave_refill(C, L, active);
    if (!active) continue;
    const bool chk = L.pos >= begin;   // an event of slice j (not of slice j - 1)
    // one read of stream st at L.pos, then the symbol
    auto rd = [&](uint32_t st) -> uint32_t {
      const uint32_t gp = SP.g[st], M = gp >> 24;
      if (L.pos + M > nb8) {
        hang = hang || (chk && (uint32_t)(L.pos & 7u) + M > 32u);
        nb8 = (L.pos + M + 7u) & ~7ull;
      }
      return dsym_gp(L, C.my, S, st, gp);
    };
    const bool at_n = q == N && (dk == 0 || closed);
    const uint32_t pfx = rd(PFX_STREAM);
    if (at_n) {
      // the extra prefix (code.rs:660); a zero digit continues the run loop
      if (dk != 0 && pfx == (uint32_t)P_RUN1) (void)pixel_count(pfx, dk);
      else active = false;
      continue;
    }
    if (pfx < (uint32_t)P_RUN1) {
      (void)rd(pay_stream(pfx, 0));
      if (pfx == (uint32_t)P_RGB || pfx == (uint32_t)P_LUMA || pfx == (uint32_t)P_LUMA2) {
        (void)rd(pay_stream(pfx, 1));
        (void)rd(pay_stream(pfx, 2));
        if (pfx == (uint32_t)P_LUMA) (void)rd(S_LUMA_OTHER);
      }
      q += 1;
      dk = 0;
      closed = false;
    } else {
      q += pixel_count(pfx, dk);
      closed = closed || q == N;
    }
  }
  if (hang) set_status(&a.status[f], NICE_E_UNSUPPORTED);
}

// ---------------------------------------------------------------------------
// D4: per-pixel records.  With every chunk's entry state and first pixel index
// known, each chunk decodes its symbols again and writes one 32-bit record per
// coded pixel, tagged with the call's tag; run pixels write nothing (a slot
// without the tag reads as REC_RUN).  A record says how the pixel follows from
// already decoded pixels (code.rs:579-644):
//   value_c = src_c + c_c (mod 256), c spread over bits 0..7, 10..17, 20..27,
//   src = floor((L + U) / 2) (L on row 0)      class 0: SMALL_DIFF, LUMA2, RGB
//   src = pixel i - off(refid)                 classes 1..13: BACK_REF (refid
//                                              0..4), LUMA (refid 5..15)
// (the layout, the tag and the class tables: nice_dec_rec.hpp).
// Records of a lane are combined into aligned groups of four and stored with
// one 16-byte store when the group lies inside the lane's pixel range.
// ---------------------------------------------------------------------------

// (make_record and its two halves, make_event_rec and rec_bad_at, are
// nice_dec_event.hpp's: dec_emit's record from a pixel's symbols.)

struct RecGroup {
  unsigned long long grp;   // first pixel of the aligned group, ~0: empty (u64: no collision with pixels)
  uint32_t v0, v1, v2, v3, mask;
  __device__ __forceinline__ void flush(uint32_t* rec, unsigned long long lo, unsigned long long hi) {
    if (!mask) return;
    if (grp >= lo && grp + 4 <= hi) {
      uint4* dst = reinterpret_cast<uint4*>(__builtin_assume_aligned(rec + grp, 16));
      *dst = make_uint4(v0, v1, v2, v3);
    } else {
      if (mask & 1u) rec[grp] = v0;
      if (mask & 2u) rec[grp + 1] = v1;
      if (mask & 4u) rec[grp + 2] = v2;
      if (mask & 8u) rec[grp + 3] = v3;
    }
  }
  __device__ __forceinline__ void put(uint32_t* rec, unsigned long long lo, unsigned long long cur,
                                      uint32_t r) {
    const unsigned long long g4 = cur & ~3ull;
    if (g4 != grp) {
      flush(rec, lo, cur);    // every pixel of the old group below cur is this lane's
      grp = g4;
      v0 = v1 = v2 = v3 = REC_RUN;
      mask = 0;
    }
    const uint32_t k = (uint32_t)(cur & 3u);
    v0 = k == 0 ? r : v0;
    v1 = k == 1 ? r : v1;
    v2 = k == 2 ? r : v2;
    v3 = k == 3 ? r : v3;
    mask |= 1u << k;
  }
};

// Lanes take sub-slices of DEC_EMIT_BITS: sub-slice s of slice j starts at the
// converged parse's checkpoint (s * DEC_EMIT_BITS / a.ck_bits - 1) -- a prefix
// position with its run digits and pixel count -- so emission parallelism does
// not depend on the slice size the sync pass uses.  With the first pass's
// events kept (a.ev), the lanes take dec_heads' list instead and each stops at
// its slice's meeting point; dec_place writes the rest.
__global__ __launch_bounds__(DEC_PARSE_THREADS) PARSE_ATTR void dec_emit(DecArgs a) {
  __shared__ LutLds S;
  __shared__ __attribute__((aligned(16))) uint32_t ring[DEC_PARSE_THREADS * RING_STRIDE];
  const uint32_t f = blockIdx.x / a.emit_blocks;
  const uint32_t vb = blockIdx.x % a.emit_blocks;
  if (a.status[f] != 0) return;
  ParseCtx C = parse_frame(a, f);
  const uint64_t D = C.D, base = C.base;
  const uint32_t subs = a.chunk_bits / DEC_EMIT_BITS;
  // with first-pass events kept, only the listed head sub-slices (dec_heads)
  const uint32_t nv = a.head_items ? a.head_count[f] : C.nc * subs;
  if (vb * DEC_PARSE_THREADS >= nv) return;
  load_lut(S, reinterpret_cast<const DecTables*>(a.tables) + f);
  __syncthreads();
  if (wave_idle(vb * DEC_PARSE_THREADS, nv)) return;
  parse_lane(C, S, ring, a, f);
  const uint32_t v = vb * DEC_PARSE_THREADS + threadIdx.x;
  const uint32_t item = !a.head_items ? v
                      : v < nv ? a.head_items[(uint64_t)f * a.max_chunks * subs + v] : 0u;
  const uint32_t j = item / subs, sub = item - j * subs;
  const uint32_t N = a.W * a.H;
  const unsigned long long begin = D + (unsigned long long)j * a.chunk_bits;
  unsigned long long q64 = 0, e = 0;
  unsigned long long end = begin + a.chunk_bits;
  bool active = v < nv;
  if (active) {
    q64 = a.chunk_start[base + j];   // pixels accounted before this slice
    const uint32_t nvalid = last_nck(a.last[base + j]);
    const unsigned long long* ck = a.ck + (uint64_t)f * a.n_ck * a.max_chunks + j;
    const uint32_t step = DEC_EMIT_BITS / a.ck_bits;
    if (sub == 0) {
      e = slice_entry(a, base, j);
    } else {
      const uint32_t c = sub * step - 1;
      if (c < nvalid) {
        const unsigned long long x = ck[(uint64_t)c * a.max_chunks];
        e = ps_pack((begin - D) + ck_pos(x), ck_dk(x));
        q64 += ck_px(x);
      } else {
        active = false;               // the slice's parse ended before this sub-slice
      }
    }
    const uint32_t c1 = (sub + 1) * step - 1;
    if (sub + 1 < subs && c1 < nvalid) end = begin + ck_pos(ck[(uint64_t)c1 * a.max_chunks]);
    if (q64 > N) active = false;      // past the image: tail bytes
    if (a.ev) {
      // dec_place writes the slice from where the final parse meets the first
      // pass (its events kept): this lane only parses the head before that,
      // and not even the head when the re-parse kept its events
      uint32_t ag, nv2, hn;
      const uint32_t route = slice_route(a, base, j, ag, nv2, hn);
      if (route == SLICE_PLACE) active = false;
      if (route == SLICE_HEAD_EMIT) {
        const unsigned long long stop = begin + ck_pos(ck[(uint64_t)(ag - 1u) * a.max_chunks]);
        if (stop < end) end = stop;
        if (sub * step >= ag) active = false;   // starts at or past the meeting point
      }
    }
  }
  uint32_t q = (uint32_t)(q64 > N ? N : q64);
  const uint32_t q0 = q;
  uint32_t* rec = a.recs + (uint64_t)f * a.rec_stride;
  const bool strict = (a.flags & NICE_DEC_STRICT_REFERENCE) != 0;
  uint32_t dk;
  Lane L = lane_at(C, e, dk);
  bool closed = (q == N);          // a run completed exactly at N earlier
  bool err = false;
  RecGroup G{~0ull, REC_RUN, REC_RUN, REC_RUN, REC_RUN, 0u};
  // one pixel event read at a prefix position: a record, a run's pixels, or
  // the end of the lane's work
  auto handle = [&](bool at_n, uint32_t pfx, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3) {
    if (at_n) {
      // a zero digit of the run that reached N: the reference's run loop
      // (code.rs:665-671) reads it and adds nothing
      if (dk != 0 && pfx == (uint32_t)P_RUN1) { (void)pixel_count(pfx, dk); return; }
      // the reference still reads one more prefix (code.rs:660): a run digit
      // there makes it copy past its buffer
      err = err || (strict && pfx >= (uint32_t)P_RUN1);
      active = false;
      return;
    }
    const uint32_t cur = q;
    const uint32_t c = pixel_count(pfx, dk);
    if (pfx < (uint32_t)P_RUN1) {
      bool bad;
      const uint32_t r = make_record(a.W, cur, pfx, s0, s1, s2, s3, bad);
      if (bad) { err = true; active = false; return; }
      G.put(rec, q0, cur, r | rec_tagbits(a.rec_tag));
      q = cur + 1;
      closed = false;
    } else {
      const unsigned long long qn = (unsigned long long)q + c;
      if (qn > N) { err = true; active = false; return; }
      q = (uint32_t)qn;
      closed = closed || q == N;
    }
  };
  // Two loops, as dec_sync: the fast parse in 32-bit positions relative to B
  // and the general symbol-by-symbol parse, which reads any tables.  The fast
  // loop is this kernel's own copy of RelCursor's: through the struct dec_emit
  // was 2-4 % slower at 64 x 1080p.
  const bool fast = parse_fast(a, f);
  const unsigned long long B = rel_base(active, L.pos, begin);
  if (fast && rel_fits(active, L.pos, B, end)) {
    const uint32_t fp_pfx = fast_param(C.SP.g[PFX_STREAM]);
    const uint32_t bwl = (uint32_t)(B >> 5);
    const uint32_t rhard = C.hard > B ? (uint32_t)min(C.hard - B, (unsigned long long)0xFFFFFFFFu) : 0u;
    const uint32_t rlim = active ? min((uint32_t)(end - B), rhard) : 0u;
    uint32_t r = active ? (uint32_t)(L.pos - B) : 0u;
    uint32_t wsr = 0, rfill = 0;
    for (;;) {
      const bool at_n = q == N && (dk == 0 || closed);   // every pixel accounted for
      if (active && r >= rlim) active = false;
      if (!__any(active)) break;
      if (__any(active && r >= rfill)) {
        const uint32_t wsa = (bwl + (r >> 5)) & ~3u;
        ring_fill_ws(C.wring, C.p, C.len, C.al16, wsa);
        wsr = wsa - bwl;
        rfill = (wsr + RING_W - 2u) << 5;
      }
      if (!active) continue;
      uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, tot;
      const uint32_t pfx = pixel_event_fast_at(C.my, S, fp_pfx, (r >> 5) - wsr, r & 31u, s0, s1, s2, s3, tot);
      r += tot;
      handle(at_n, pfx, s0, s1, s2, s3);
    }
  } else {
    for (;;) {
      // at a prefix position
      const bool at_n = q == N && (dk == 0 || closed);   // every pixel accounted for
      if (active && (L.pos >= end || L.pos >= C.hard)) active = false;
      if (!__any(active)) break;
      (void)wave_refill(C, L, active);
      if (!active) continue;
      uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
      const uint32_t pfx = pixel_event(L, C.my, S, C.SP, s0, s1, s2, s3);
      handle(at_n, pfx, s0, s1, s2, s3);
    }
  }
  G.flush(rec, q0, q0);   // last group: per-record stores (the next lane may own the rest)
  if (err) set_status(&a.status[f], NICE_E_FORMAT);
}

// ---------------------------------------------------------------------------
// D4a: list the sub-slices dec_emit parses (one 1024-thread block per frame):
// each slice's head before the checkpoint where the final parse meets the
// first pass, or the whole slice when it never does (or its events
// overflowed).  Compact lists keep dec_emit's waves full of working lanes.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void dec_heads(DecArgs a) {
  __shared__ uint32_t part[1024];
  const uint32_t f = blockIdx.x;
  if (a.status[f] != 0) {
    if (threadIdx.x == 0) a.head_count[f] = 0;
    return;
  }
  const uint32_t nc = n_chunks(a.stream_len[f], a.data_start[f], a.chunk_bits);
  const uint64_t base = (uint64_t)f * a.max_chunks;
  const uint32_t subs = a.chunk_bits / DEC_EMIT_BITS, step = DEC_EMIT_BITS / a.ck_bits;
  const uint32_t per = (nc + 1023) / 1024;
  const uint32_t c0 = min(threadIdx.x * per, nc), c1 = min(c0 + per, nc);
  auto nsub = [&](uint32_t j) -> uint32_t {
    uint32_t ag, nvalid, hn;
    const uint32_t route = slice_route(a, base, j, ag, nvalid, hn);
    if (route == SLICE_EMIT) return min(subs, 1u + nvalid / step);   // every sub-slice with a start (s * step - 1 < nvalid)
    if (route == SLICE_PLACE) return 0u;      // dec_place has the head's events
    return (ag + step - 1) / step;            // sub-slices starting before the meeting point
  };
  uint32_t cnt = 0;
  for (uint32_t j = c0; j < c1; ++j) cnt += nsub(j);
  part[threadIdx.x] = cnt;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint32_t t = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
    __syncthreads();
    part[threadIdx.x] += t;
    __syncthreads();
  }
  uint32_t o = part[threadIdx.x] - cnt;
  uint32_t* items = a.head_items + base * subs;
  for (uint32_t j = c0; j < c1; ++j) {
    const uint32_t n = nsub(j);
    for (uint32_t s = 0; s < n; ++s) items[o++] = j * subs + s;
  }
  if (threadIdx.x == 1023) a.head_count[f] = part[1023];
}

// ---------------------------------------------------------------------------
// D4b: place each slice's kept events (one wave per slice): the head's, kept
// by the slice's latest re-parse, from the slice's first pixel, then the first
// pass's past the meeting point; pixel positions by a wave prefix sum of the events' pixel
// counts, one coalesced 4-byte record store per coded pixel, runs left to the
// memset marker.  Same checks as dec_emit: the first event at q == N is the
// extra prefix the reference reads (strict: a run digit there is an error),
// a run past N or a reference the reference rejects sets NICE_E_FORMAT.
// ---------------------------------------------------------------------------
// The record comes from the event word by place_record (nice_dec_event.hpp):
// masks from a table entry per (reference id, prefix) instead of compares and
// selects on the prefix, the SMALL_DIFF constant from a table (kSdl in LDS).
__device__ __constant__ SdlTable kSdl = make_sdl_table();

__global__ __launch_bounds__(64 * DEC_PLACE_WAVES) void dec_place(DecArgs a) {
  // kSdl (code.rs:230-247), zero up to the 512 words a 9-bit index reaches (a
  // run event's count bits, read as a SMALL_DIFF index, stay inside)
  __shared__ __attribute__((aligned(16))) uint32_t sdl[512];
  __shared__ PlaceEnt idt[PLACE_ENTRIES];   // (reference id, prefix) -> class and masks (place_entry)
  __shared__ uint32_t off3[PLACE_ENTRIES];  // ... -> pixels needed before the event + 3 (the checked steps)
  static_assert(64 * DEC_PLACE_WAVES >= PLACE_ENTRIES + 128, "one thread per table entry");
  if (threadIdx.x >= 64u * DEC_PLACE_WAVES - PLACE_ENTRIES) {   // (the threads that do not fill sdl)
    const uint32_t entry = threadIdx.x - (64u * DEC_PLACE_WAVES - PLACE_ENTRIES);
    uint32_t o3;
    idt[entry] = place_entry(entry, a.W, o3);
    off3[entry] = o3;
  }
  // copied from a compile-time table: computing the 343 constants in every
  // block (divisions by 7 and 49) cost ~120 VALU per wave, and dec_place runs
  // one short-lived block per four slices
  if (threadIdx.x < 86u)
    reinterpret_cast<uint4*>(sdl)[threadIdx.x] = reinterpret_cast<const uint4*>(kSdl.v)[threadIdx.x];
  else if (threadIdx.x < 128u)
    reinterpret_cast<uint4*>(sdl)[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  // grid (slices / waves, frames), XCD-aware: consecutive logical blocks are
  // dealt to one XCD (blocks b and b + 8 share one; bijective remap, guide T1),
  // so the two blocks whose slices share each 128-byte event line (8 slices'
  // 16-byte quads, interleaved per parse wave) read it through one L2
  const uint32_t nbx = gridDim.x, nwg = nbx * gridDim.y, lin = blockIdx.y * nbx + blockIdx.x;
  const uint32_t xq = nwg / 8u, xr = nwg % 8u, xcd = lin % 8u;
  const uint32_t lg = (xcd < xr ? xcd * (xq + 1u) : xr * (xq + 1u) + (xcd - xr) * xq) + lin / 8u;
  // (the wave's slice in a scalar register: its bookkeeping and the event
  // buffers' bases then take no vector registers)
  const uint32_t f = lg / nbx, j = (lg % nbx) * DEC_PLACE_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (a.status[f] != 0) return;
  const uint64_t len = a.stream_len[f];
  const uint64_t D = a.data_start[f];
  if (j >= n_chunks(len, D, a.chunk_bits)) return;
  const uint64_t base = (uint64_t)f * a.max_chunks;
  uint32_t ag, nvalid, hn;
  const uint32_t route = slice_route(a, base, j, ag, nvalid, hn);
  const uint32_t nev = a.ev_n[base + j];
  if (a.stats && lane == 0) {   // diagnostics: where the final parse met the first pass
    const uint32_t b = nev == EV_OVERFLOW ? 7u : ag == AGREE_NONE ? 6u : ag == 0u ? 0u : ag == 1u ? 1u
                     : ag <= 4u ? 2u : ag <= 16u ? 3u : ag <= 64u ? 4u : 5u;
    atomicAdd(&a.stats[50 + b], 1ull);
    // the slice's head: none (the first pass started at the final entry),
    // placed here, parsed by dec_emit, or the whole slice parsed by dec_emit
    atomicAdd(&a.stats[route == SLICE_EMIT ? 29 : route == SLICE_HEAD_EMIT ? 28 : ag == 0u ? 26 : 27], 1ull);
  }
  if (route == SLICE_EMIT) return;   // dec_emit parsed it all
  // the head's events kept by the latest re-parse (hn of them), then the first
  // pass's from the meeting checkpoint.  (One index space over both buffers,
  // each lane picking buffer and index, cost dec_place 28 % for 10 % more
  // events: 15 more VGPRs and a 64-bit select per load.  The two are walked
  // one after the other instead, every step reading one buffer.)
  const bool head = route == SLICE_PLACE && ag != 0u;
  // (the bookkeeping loads issued together, the first checkpoint taken as
  // the meeting point before `agree` is in: no faster, r06zv_ab_pack_place.log)
  const uint64_t cki = (uint64_t)f * a.n_ck * a.max_chunks + j + (uint64_t)(ag ? ag - 1u : 0u) * a.max_chunks;
  // (wave-uniform values the tail needs after the head's loop, kept in scalar registers)
  auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
  const uint32_t i_first1 = uni(ag == 0u ? 0u : a.ev_ck[cki]), nev1 = uni(nev);
  hn = uni(hn);
  const unsigned long long q_first = a.chunk_start[base + j];
  // pixels before the meeting point: where the head's events must end
  const unsigned long long q_meet_v = q_first + (ag == 0u ? 0ull : ck_px(a.ck[cki]));
  const unsigned long long q_meet = ((unsigned long long)uni((uint32_t)(q_meet_v >> 32)) << 32) | uni((uint32_t)q_meet_v);
  unsigned long long q = head ? q_first : q_meet;
  const uint64_t N = (uint64_t)a.W * a.H;
  if (q > N) return;                    // tail bytes
  // place_deep in 32 bits (q <= N <= 2^30): never, for a row that wide
  const uint32_t deep32 = 3ull * a.W + 3u > 0xFFFFFFFFull ? 0xFFFFFFFFu : 3u * a.W + 3u;
  uint32_t* rec = a.recs + (uint64_t)f * a.rec_stride;
  const bool strict = (a.flags & NICE_DEC_STRICT_REFERENCE) != 0;
  bool err = false, stopped = false;
  for (uint32_t part = head ? 0u : 1u; part < 2u && !stopped; ++part) {
  // events [i_first, nev) of this part's buffer
  const uint32_t* evp = part == 0u ? a.hev + ev_group(a, f, j, a.hev_cap) : a.ev + ev_group(a, f, j, a.ev_cap);
  const uint32_t i_first = part == 0u ? 0u : i_first1, nev = part == 0u ? hn : nev1;
  if (part == 1u && head && q != q_meet) {
    // the head must end where the first pass's events take over, or the two
    // parses are not the ones the checkpoints describe: the frame fails
    // (NICE_E_HIP, as a parse that is not at its fixpoint), never decodes
    if (lane == 0) {
      if (a.stats) atomicAdd(&a.stats[30], 1ull);
      set_status(&a.status[f], NICE_E_HIP);
    }
    return;
  }
  // 256 events per step: 4 rows of 64 consecutive events (coalesced loads and
  // record stores), prefix sums per row plus the rows before
  // the next step's events, loaded one step ahead and unconditionally (lanes
  // past the slice's last event read that event again and are masked where
  // used): with every load issued, the compiler's wait at the top of a step
  // leaves the next step's four in flight (a conditional load with a zero
  // fill made it wait for all of them)
  if (i_first >= nev) continue;
  const uint32_t ev_last = nev - 1u;
  uint32_t nx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) nx[k] = evp[ev_word(min(i_first + 64u * k + lane, ev_last))];
  for (uint32_t i = i_first; i < nev; i += 256u) {
    uint32_t ev[4], r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ev[k] = nx[k];
      nx[k] = evp[ev_word(min(i + 256u + 64u * k + lane, ev_last))];
    }
    // fast path (nearly every step): every count < 2^16, so positions and
    // sums stay 32-bit (q <= N <= 2^30), and no event reaches the frame end or
    // carries a bad reference -- one uniform check, then plain stores
    {
      const uint32_t N32 = (uint32_t)N;
      // (wave-uniform) past every reference's reach and the first row: the
      // step's records take no position check
      const bool deep = uni((uint32_t)q) >= deep32;
      uint32_t c32[4];
      bool big = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool valid = i + 64u * k + lane < nev;
        c32[k] = valid ? ((ev[k] & EV_RUN) ? (ev[k] & ~EV_RUN) : 1u) : 0u;
        big = big || c32[k] >= 65536u;
      }
      if (!__any(big)) {
        uint32_t qb[4];
        uint32_t base = (uint32_t)q;
        bool stop = false;
        auto rows = [&](auto check_tag) {
          constexpr bool CHECK = decltype(check_tag)::value;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            // rows past the slice's last event (a slice's last step is mostly
            // empty): skipped by a uniform branch, not computed under a mask
            if (i + 64u * k >= nev) break;
            const bool valid = i + 64u * k + lane < nev;
            const bool run = (ev[k] & EV_RUN) != 0u;
            const uint32_t incl = wave_incl_scan(c32[k]);
            qb[k] = base + incl - c32[k];
            base += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            bool rbad = false;
            r[k] = place_record<CHECK>(ev[k], min(qb[k], N32), sdl, idt, off3, rbad);
            stop = stop || (valid && (qb[k] >= N32 || (run ? qb[k] + c32[k] > N32 : rbad)));
          }
        };
        if (deep) rows(std::false_type{});
        else rows(std::true_type{});
        if (!__any(stop)) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (i + 64u * k >= nev) break;
            if (i + 64u * k + lane < nev && !(ev[k] & EV_RUN)) rec[qb[k]] = r[k] | rec_tagbits(a.rec_tag);
          }
          q = base;
          continue;
        }
      }
    }
    // exact path: 64-bit positions, the first event at the frame end or in error stops
    unsigned long long c[4], qk[4], carry = 0;
    uint32_t stop_k = 4u, stop_lane = 64u;
    bool stop_at_n = false, stop_run = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t x = i + 64u * k + lane;
      const bool valid = x < nev;
      const bool run = (ev[k] & EV_RUN) != 0u;
      c[k] = valid ? (run ? (ev[k] & ~EV_RUN) : 1u) : 0u;
      unsigned long long incl;
      if (!__any(c[k] >= (1u << 25))) {   // 64 counts < 2^25: a 32-bit scan
        incl = wave_incl_scan((uint32_t)c[k]);
      } else {
        incl = c[k];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned long long t = __shfl_up(incl, o);
          if ((int)lane >= o) incl += t;
        }
      }
      const unsigned long long qb = q + carry + incl - c[k];   // pixels before this event
      carry += __shfl(incl, 63);
      qk[k] = qb;
      bool rbad = false;
      r[k] = place_record<true>(ev[k], (uint32_t)min(qb, N), sdl, idt, off3, rbad);
      // a zero-count run event is a zero digit continuing a run (the first
      // digit counts >= 1): at N the reference's run loop reads it and goes on
      const bool at_n = valid && qb == N && !(run && c[k] == 0);
      const bool bad = valid && !at_n && (run ? qb + c[k] > N : rbad);
      const unsigned long long m = __ballot(at_n || bad);
      if (stop_k == 4u && m) {
        stop_k = (uint32_t)k;
        stop_lane = (uint32_t)__builtin_ctzll(m);
        stop_at_n = __shfl(at_n ? 1 : 0, (int)stop_lane) != 0;
        stop_run = __shfl(run ? 1 : 0, (int)stop_lane) != 0;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool keep = (uint32_t)k < stop_k || ((uint32_t)k == stop_k && lane < stop_lane);
      if (keep && i + 64u * k + lane < nev && !(ev[k] & EV_RUN)) rec[qk[k]] = r[k] | rec_tagbits(a.rec_tag);
    }
    if (stop_k < 4u) {
      if (lane == 0) err = stop_at_n ? (strict && stop_run) : true;
      stopped = true;
      break;
    }
    q += carry;
  }
  }
  if (err) set_status(&a.status[f], NICE_E_FORMAT);
}


}  // namespace nice
