// nice_capi.hip -- host runtime behind include/nice.h: contexts, scratch arenas,
// kernel launch sequences and the host-buffer convenience entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <cmath>
#include <mutex>
#include <algorithm>
#include <vector>

#include "../../include/nice.h"
#include "../../include/nice_test.h"
#include "nice_format.h"
#include "nice_bits.hpp"
#include "nice_kernels.h"
#include "nice_dec_plan.hpp"
#include "nice_enc_plan.hpp"
#include "nice_slot_plan.hpp"
#include "nice_rec.hpp"
#include "nice_resize.hpp"
#include "nice_tiles.hpp"
#include "nice_internal.h"

using namespace nice;

#define NICE_HIP(x)                          \
  do {                                       \
    if ((x) != hipSuccess) return NICE_E_HIP; \
  } while (0)

namespace {

// Device scratch arena, grown on demand (reserve() to pre-size).
struct Arena {
  void* ptr = nullptr;
  size_t cap = 0;
  uint64_t gen = 0;   // bumped by every (re)allocation: contents are unknown after it
  int grow(size_t bytes) {
    if (bytes <= cap) return NICE_OK;
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    ++gen;
    if (hipMalloc(&ptr, bytes) != hipSuccess) return NICE_E_HIP;
    cap = bytes;
    return NICE_OK;
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Test / A/B options (include/nice_test.h; nice_test_set_option): stored as
// value + 1, 0 = unset.  Nothing in the library reads the environment.
std::atomic<int64_t> g_opt[NICE_OPT_COUNT];
inline bool opt_set(int id) { return g_opt[id].load(std::memory_order_relaxed) != 0; }
inline int64_t opt_val(int id) { return g_opt[id].load(std::memory_order_relaxed) - 1; }
inline bool opt_on(int id) { return opt_set(id) && opt_val(id) != 0; }

// Encoder scratch layout. The zero-per-launch block comes first (memset once).
struct EncLayout {
  size_t zero_bytes, total;
  size_t o_hist, o_flags, o_ctr, o_status, o_overn, o_overl;
  size_t o_first, o_last, o_next, o_tblcode, o_len8, o_smax, o_seedbit, o_recs, o_tbits, o_toff, o_dend, o_packtab,
      o_gacc, o_bhist, o_cmask;
};

EncLayout enc_layout(uint32_t n_frames, uint32_t T, uint64_t npx) {
  EncLayout L{};
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
  L.o_hist = take((size_t)n_frames * N_BINS * 4);
  L.o_flags = take((size_t)n_frames * 4 + 4);   // + one word: any frame FLAG_LONG
  L.o_ctr = take((size_t)n_frames * 4);
  L.o_status = take((size_t)n_frames * T * 8);
  L.o_overn = take(4);
  L.zero_bytes = align_up(o, 16);
  L.o_overl = take((size_t)n_frames * ((T + PACK_SUB - 1) / PACK_SUB) * 8);
  L.o_first = take((size_t)n_frames * T * 4);
  L.o_last = take((size_t)n_frames * T * 4);
  L.o_next = take((size_t)n_frames * T * 4);
  L.o_tblcode = take((size_t)n_frames * N_BINS * 4);
  L.o_len8 = take((size_t)n_frames * N_BINS);
  L.o_smax = take((size_t)n_frames * N_STREAMS);
  L.o_seedbit = take((size_t)n_frames * 8);
  L.o_recs = take((size_t)n_frames * ((npx + 3) & ~3ull) * 4);
  L.o_tbits = take((size_t)n_frames * T * 4);
  L.o_toff = take((size_t)n_frames * T * 8);
  L.o_dend = take((size_t)n_frames * 8);
  L.o_packtab = take((size_t)n_frames * sizeof(PackTab));
  L.o_gacc = take((size_t)n_frames * ((T + ENC_GROUP_TILES - 1) / ENC_GROUP_TILES + 1) * 8);
  L.o_bhist = take((size_t)N_BINS * 4);   // band API: the band's own histogram
  L.o_cmask = take((size_t)n_frames * T * (ENC_TILE / 32) * 4);   // 1 bit per pixel
  L.total = o;
  return L;
}

int check_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= device || device < 0) return NICE_E_NODEV;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return NICE_E_NODEV;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return NICE_E_NODEV;
  return NICE_OK;
}

}  // namespace

static const char* kPhaseNames[NICE_PHASES] = {
    "enc_classify", "enc_tailruns", "enc_tables", "enc_header", "enc_tilebits", "enc_tilescan",
    "enc_pack", "enc_tail", "enc_pack_long", "dec_tables", "dec_sync", "dec_scan", "dec_emit",
    "dec_reconstruct", "dec_place", "dec_resync"};

// Optional per-phase HIP-event timing (bench / profiling).
struct PhaseTimer {
  bool on = false;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  struct Mark { int phase; hipEvent_t a, b; };
  std::vector<Mark> marks;
  hipEvent_t take() {
    if (used == pool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      pool.push_back(e);
    }
    return pool[used++];
  }
  void begin(int phase, hipStream_t st) {
    if (!on) return;
    Mark m{phase, take(), take()};
    if (!m.a || !m.b) return;
    (void)hipEventRecord(m.a, st);
    marks.push_back(m);
  }
  void end(hipStream_t st) {
    if (!on || marks.empty()) return;
    (void)hipEventRecord(marks.back().b, st);
  }
  void release() {
    for (auto e : pool) (void)hipEventDestroy(e);
    pool.clear();
    marks.clear();
    used = 0;
  }
};

struct BandState {
  bool classified = false, tabled = false;
  nice::EncArgs a{};
  nice::EncPlan plan{};   // of the band's classify, runs and pack
  uint64_t band_bits = 0, seed_bit = 0;
  // the band's own symbol counts (nice_band_runs), for its bit count
  uint32_t* bhist = nullptr;
  // nice_band_tables_dev's {band bits, data start}, copied into the context
  // (band_hdr): the pack compares the caller's band_bits with it
  const unsigned long long* d_info = nullptr;
};

struct nice_ctx {
  int device = 0;
  std::mutex mu;
  Arena enc, dec, host_px, host_out, dev_len, band, band_hdr;
  Arena pack;   // nice_encode_batch_packed_dev: the strided streams before they are packed
  // tiled images: the split tiles, the decoded tiles, and the small tables
  // (gathered offsets, tile indices, statuses) of one call
  Arena tiles, tile_dec, tile_tab;
  Arena aa_weights;                                     // the weight tables of the antialiased resize
  uint32_t last_tiled_coded = 0, last_tiled_raw = 0;   // test hook nice_test_last_tiled
  uint32_t last_set_coded = 0, last_set_raw = 0;       // test hook nice_test_last_set
  uint32_t last_set_merges = 0;                         // test hook nice_test_last_set_merges
  uint32_t last_set_alpha_coded = 0, last_set_alpha_raw = 0, last_set_alpha_const = 0;   // nice_test_last_set_alpha
  PhaseTimer timer;
  BandState bs;
  // decoder record tags (DecArgs::rec_tag): the region the last call used and its tag
  uint32_t* rec_region = nullptr;
  uint64_t rec_words = 0, rec_gen = 0;
  uint32_t rec_epoch = 0;
  int cus = 0;   // compute units of the device (enc_pack's persistent grid)
  // the last split decode's per-frame abort flags (test hook nice_test_split_redos)
  const uint32_t* split_abort = nullptr;
  uint32_t split_frames = 0;
  // DecRoute of the last decode's row kernel and of its redo launch (test hook nice_test_last_dec_route)
  uint32_t last_dec_route = 0, last_dec_fallback = 0;
  int last_classify = -1;  // ClsKind of the last encode / band classify (test hook nice_test_last_classify)
  // test hooks (nice_test_set_hooks; 0 = off): the last strip of every split
  // decode returns at entry; enc_pack's LDS group buffer in bits per pixel
  uint32_t test_split_absent = 0, test_pack_cap_bpp = 0;
};

extern "C" {

const char* nice_version(void) { return "nice-mi355x 0.1 (gfx950)"; }

int nice_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

size_t nice_encode_bound(uint32_t w, uint32_t h) {
  // Huffman cost <= fixed-length cost per stream: <= 28 bits per coded pixel,
  // <= 2 bits per run pixel for digits (code.rs:391-406). Table header <= 858
  // 8-bit fields + 10 5-bit fields. 32 bits/px keeps it simple and word aligned.
  return (size_t)FILE_HEADER_BYTES + 880 + (size_t)w * h * 4 + 32;
}

int nice_peek_header(const uint8_t* s, size_t len, uint32_t* w, uint32_t* h, uint8_t* ch) {
  if (!s || len < 13) return NICE_E_FORMAT;
  if (w) *w = ((uint32_t)s[4] << 24) | ((uint32_t)s[5] << 16) | ((uint32_t)s[6] << 8) | s[7];
  if (h) *h = ((uint32_t)s[8] << 24) | ((uint32_t)s[9] << 16) | ((uint32_t)s[10] << 8) | s[11];
  if (ch) *ch = s[12];
  return NICE_OK;
}

int nice_ctx_create(int device, nice_ctx** out) {
  if (!out) return NICE_E_ARG;
  int rc = check_device(device);
  if (rc) return rc;
  nice_ctx* c = new nice_ctx();
  c->device = device;
  hipDeviceProp_t prop;
  c->cus = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256;
  *out = c;
  return NICE_OK;
}

void nice_ctx_destroy(nice_ctx* ctx) {
  if (!ctx) return;
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(ctx->device);
  ctx->enc.release();
  ctx->dec.release();
  ctx->host_px.release();
  ctx->host_out.release();
  ctx->dev_len.release();
  ctx->band.release();
  ctx->band_hdr.release();
  ctx->pack.release();
  ctx->tiles.release();
  ctx->tile_dec.release();
  ctx->tile_tab.release();
  ctx->aa_weights.release();
  ctx->timer.release();
  (void)hipSetDevice(prev);
  delete ctx;
}

int nice_ctx_reserve(nice_ctx* ctx, uint32_t n_frames, uint32_t w, uint32_t h) {
  return nice::ctx_reserve_impl(ctx, n_frames, w, h, true);
}

}  // extern "C"

// nice_encode_batch_packed_dev's strided scratch: one slot per frame
static uint64_t packed_slot_bytes(uint32_t w, uint32_t h) { return align_up(nice_encode_bound(w, h), 256); }

int nice::ctx_reserve_impl(nice_ctx* ctx, uint32_t n_frames, uint32_t w, uint32_t h, bool with_packed) {
  if (!ctx) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  EncLayout L = enc_layout(n_frames, enc_tiles(w, h), (uint64_t)w * h);
  int rc = ctx->enc.grow(L.total);
  if (rc == NICE_OK && with_packed) rc = ctx->pack.grow((size_t)n_frames * packed_slot_bytes(w, h));
  return rc;
}

namespace {
// The kernel arguments of a plan: scratch pointers from the layout, the plan's
// launch-dependent fields (tile range, groups, tiles per block, pack slots).
EncArgs enc_args(const nice_ctx* ctx, const EncLayout& L, uint8_t* base, const EncPlan& p, uint32_t n_frames,
                 uint32_t w, uint32_t h, uint8_t channels, uint8_t channels_out) {
  const uint64_t N = (uint64_t)w * h;
  const uint32_t T = p.tiles_per_frame;
  EncArgs a{};
  a.n_frames = n_frames;
  a.W = w;
  a.H = h;
  a.C = channels;
  a.channels_out = channels_out;
  a.tiles_per_frame = T;
  a.tiles_per_block = p.tiles_per_block;
  a.hist = (uint32_t*)(base + L.o_hist);
  a.frame_flags = (uint32_t*)(base + L.o_flags);
  a.tile_first = (uint32_t*)(base + L.o_first);
  a.tile_last = (uint32_t*)(base + L.o_last);
  a.tile_next = (uint32_t*)(base + L.o_next);
  a.cmask = p.flags_out ? (uint32_t*)(base + L.o_cmask) : nullptr;
  a.cmask_std = p.cmask_std;
  a.tbl_code = (uint32_t*)(base + L.o_tblcode);
  a.tbl_len8 = base + L.o_len8;
  a.stream_max = base + L.o_smax;
  a.seed_bit = (unsigned long long*)(base + L.o_seedbit);
  a.recs = (uint32_t*)(base + L.o_recs);
  a.rec_stride = (N + 3) & ~3ull;
  a.tile_bits = (uint32_t*)(base + L.o_tbits);
  a.packtab = base + L.o_packtab;
  a.pack_ctr = (uint32_t*)(base + L.o_ctr);
  a.pack_slots = p.pack_slots;
  a.status = (unsigned long long*)(base + L.o_status);
  a.tile_off = (unsigned long long*)(base + L.o_toff);
  a.data_end = (unsigned long long*)(base + L.o_dend);
  a.tile_lo = p.tile_lo;
  a.tile_hi = p.tile_hi;
  a.groups = p.groups;
  a.gacc = (unsigned long long*)(base + L.o_gacc);
  a.px_lo = 0;
  a.px_hi = (int64_t)N;
  a.band = 0;
  a.over_count = (uint32_t*)(base + L.o_overn);
  a.over_list = (uint2*)(base + L.o_overl);
  a.pack_cap_bits = (uint32_t)PACK_SUB * ENC_TILE * (ctx->test_pack_cap_bpp ? ctx->test_pack_cap_bpp : NICE_PACK_CAP_BPP);
  return a;
}

EncOpts enc_opts() {
  return EncOpts{opt_on(NICE_OPT_ENC_NO_RING), opt_on(NICE_OPT_ENC_NO_PAIR), opt_on(NICE_OPT_ENC_NO_SLIDE)};
}

// The classify kernels: -1 matches either value.  A plan without an entry
// (there is no RGB strip, pair or slide kernel) is an error, never another kernel.
struct ClsEntry {
  ClsKind kind;
  int rgb, flags_out, wmod4;
  void (*fn)(EncArgs);
};
const ClsEntry kClassify[] = {
    {CLS_K_WINDOW, -1, -1, -1, enc_classify},
    {CLS_K_TINY, -1, -1, -1, enc_classify_tiny},
    {CLS_K_RING, 0, 0, -1, enc_classify_ring},
    {CLS_K_RING, 0, 1, -1, enc_classify_ring_m},
    {CLS_K_RING, 1, 0, -1, enc_classify_ring3},
    {CLS_K_RING, 1, 1, -1, enc_classify_ring3_m},
    {CLS_K_RING2, 0, 0, -1, enc_classify_ring2},
    {CLS_K_RING2, 0, 1, -1, enc_classify_ring2_m},
    {CLS_K_RING2, 1, 0, -1, enc_classify_ring2_3},
    {CLS_K_RING2, 1, 1, -1, enc_classify_ring2_3_m},
    {CLS_K_STRIP, 0, 0, -1, enc_classify_strip},
    {CLS_K_STRIP, 0, 1, -1, enc_classify_strip_m},
    {CLS_K_PAIR, 0, 0, -1, enc_classify_pair},
    {CLS_K_PAIR, 0, 1, -1, enc_classify_pair_m},
    {CLS_K_TWIN, 0, 0, -1, enc_classify_twin},
    {CLS_K_TWIN, 0, 1, -1, enc_classify_twin_m},
    {CLS_K_TWIN, 1, 0, -1, enc_classify_twin3},
    {CLS_K_TWIN, 1, 1, -1, enc_classify_twin3_m},
    {CLS_K_SLIDE, 0, 1, 0, enc_classify_slide0},   // frames only: coded flags out in ballot order
    {CLS_K_SLIDE, 0, 1, 1, enc_classify_slide1},
    {CLS_K_SLIDE, 0, 1, 2, enc_classify_slide2},
    {CLS_K_SLIDE, 0, 1, 3, enc_classify_slide3},
};

inline dim3 grid_of(const EncLaunch& l) { return dim3(l.x, l.y); }

// Classify and, for frames, the in-tile run digits from the coded flags.
int launch_classify(const EncPlan& p, const EncArgs& a, hipStream_t st) {
  auto is = [](int want, int got) { return want < 0 || want == got; };
  for (const ClsEntry& e : kClassify) {
    if (e.kind != p.kind || !is(e.rgb, p.rgb) || !is(e.flags_out, p.flags_out) || !is(e.wmod4, (int)p.wmod4)) continue;
    hipLaunchKernelGGL(e.fn, grid_of(p.classify), dim3(p.classify.threads), 0, st, a);
    if (p.rundigits.on())
      hipLaunchKernelGGL(enc_rundigits, grid_of(p.rundigits), dim3(p.rundigits.threads), 0, st, a, p.il);
    return NICE_OK;
  }
  return NICE_E_ARG;
}

// Runs crossing tile ends: the groups' first coded pixels, then the tail runs.
void launch_runs(const EncPlan& p, const EncArgs& a, hipStream_t st) {
  if (p.group_reduce.on())
    hipLaunchKernelGGL(enc_group_reduce, grid_of(p.group_reduce), dim3(p.group_reduce.threads), 0, st, a, 0);
  hipLaunchKernelGGL(enc_tailruns, grid_of(p.tailruns), dim3(p.tailruns.threads), 0, st, a);
}

// Bit placement.  tm: the frames' phase timer, or null (bands).
void launch_pack(const EncPlan& p, const EncArgs& a, hipStream_t st, PhaseTimer* tm) {
  auto begin = [&](int phase) { if (tm) tm->begin(phase, st); };
  auto end = [&]() { if (tm) tm->end(st); };
  // frames (bands) with codes over 25 bits or composed entries over 32
  // (FLAG_LONG; the launches return at once for the others): tile bits, their
  // scan, codes that fit the cache, then the wrapped writes
  begin(NICE_PH_ENC_LONG);
  hipLaunchKernelGGL(enc_tilebits, grid_of(p.long_path), dim3(p.long_path.threads), 0, st, a);
  if (p.group_reduce.on())
    hipLaunchKernelGGL(enc_group_reduce, grid_of(p.group_reduce), dim3(p.group_reduce.threads), 0, st, a, 1);
  hipLaunchKernelGGL(enc_tilescan, grid_of(p.tilescan), dim3(p.tilescan.threads), 0, st, a);
  hipLaunchKernelGGL(enc_pack_long, grid_of(p.long_path), dim3(p.long_path.threads), 0, st, a, 0);
  hipLaunchKernelGGL(enc_pack_long, grid_of(p.long_path), dim3(p.long_path.threads), 0, st, a, 1);
  end();
  // every other frame (band): one pass, group offsets by look-back
  begin(NICE_PH_ENC_PACK);
  hipLaunchKernelGGL(enc_pack, grid_of(p.pack), dim3(p.pack.threads), 0, st, a);
  hipLaunchKernelGGL(enc_pack_over, grid_of(p.pack_over), dim3(p.pack_over.threads), 0, st, a);
  hipLaunchKernelGGL(enc_edges, grid_of(p.edges), dim3(p.edges.threads), 0, st, a);
  end();
}
}  // namespace

extern "C" {

int nice_encode_batch_dev(nice_ctx* ctx, void* stream, const uint8_t* d_px, uint64_t frame_stride,
                          uint32_t n_frames, uint32_t w, uint32_t h, uint8_t channels,
                          uint8_t channels_out, uint8_t* d_out, uint64_t out_stride,
                          uint64_t* d_out_len) {
  if (!ctx || !d_out || !d_out_len) return NICE_E_ARG;
  if (channels != 3 && channels != 4) return NICE_E_ARG;
  const uint64_t N = (uint64_t)w * h;
  if (N > (1ull << 30)) return NICE_E_ARG;
  if (n_frames == 0) return NICE_OK;
  if (N > 0 && !d_px) return NICE_E_ARG;
  if (out_stride < nice_encode_bound(w, h) || (out_stride & 3) || ((uintptr_t)d_out & 3))
    return NICE_E_ARG;
  if (channels == 4 && N > 0 && (((uintptr_t)d_px & 3) || (frame_stride & 3))) return NICE_E_ARG;
  if (N > 0 && frame_stride < N * channels) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const uint32_t T = enc_tiles(w, h);
  if ((uint64_t)n_frames * T >= (1ull << 32)) return NICE_E_ARG;   // enc_pack's 32-bit work counter
  EncShape shape{};
  shape.n_frames = n_frames;
  shape.w = w;
  shape.h = h;
  shape.channels = channels;
  shape.cus = ctx->cus;
  // one frame: its stride is never applied (an odd W*H*3 RGB stride is fine)
  shape.aligned4 = ((uintptr_t)d_px & 3) == 0 && (n_frames == 1 || (frame_stride & 3) == 0);
  shape.aligned16 = ((uintptr_t)d_px & 15) == 0 && (n_frames == 1 || (frame_stride & 15) == 0);
  const EncPlan P = plan_encode(shape, enc_opts());
  EncLayout L = enc_layout(n_frames, T, N);
  int rc = ctx->enc.grow(L.total);
  if (rc) return rc;
  uint8_t* base = (uint8_t*)ctx->enc.ptr;
  EncArgs a = enc_args(ctx, L, base, P, n_frames, w, h, channels, channels_out);
  a.px = d_px;
  a.frame_stride = frame_stride;
  a.out = d_out;
  a.out_stride = out_stride;
  a.out_len = (unsigned long long*)d_out_len;
  NICE_HIP(hipMemsetAsync(base, 0, L.zero_bytes, st));
  PhaseTimer& tm = ctx->timer;
  if (T > 0) {
    tm.begin(NICE_PH_ENC_CLASSIFY, st);
    if ((rc = launch_classify(P, a, st))) return rc;
    ctx->last_classify = (int)P.kind;
    tm.end(st);
    tm.begin(NICE_PH_ENC_TAILRUNS, st);
    launch_runs(P, a, st);
    tm.end(st);
  }
  tm.begin(NICE_PH_ENC_TABLES, st);
  hipLaunchKernelGGL(enc_tables, grid_of(P.tables), dim3(P.tables.threads), 0, st, a);
  tm.end(st);
  tm.begin(NICE_PH_ENC_HEADER, st);
  hipLaunchKernelGGL(enc_header, grid_of(P.header), dim3(P.header.threads), 0, st, a);
  tm.end(st);
  if (T > 0) {
    tm.begin(NICE_PH_ENC_TILEBITS, st);
    hipLaunchKernelGGL(enc_packtab, grid_of(P.packtab), dim3(P.packtab.threads), 0, st, a);
    tm.end(st);
    launch_pack(P, a, st, &tm);
    tm.begin(NICE_PH_ENC_TAIL, st);
    hipLaunchKernelGGL(enc_tail, grid_of(P.tail), dim3(P.tail.threads), 0, st, a);
    tm.end(st);
  }
  NICE_HIP(hipGetLastError());
  return NICE_OK;
}


// ---- decoder ---------------------------------------------------------------
namespace {
struct DecLayout {
  size_t total;
  size_t o_tables, o_dstart, o_entry, o_last, o_ck, o_cpx, o_cstart, o_recs, o_changed, o_fchanged, o_rowbuf;
  size_t o_ev, o_evck, o_evn, o_agree, o_items, o_icount;
  size_t o_hev, o_hevn, o_hevag;
  size_t o_hand, o_abort;
};
// Jacobi iterations queued (one change flag each; each returns at once when the
// previous one changed nothing), then the device-side settle (dec_sync_settle)
// and one more iteration behind its flag: no host round trip.  Flags: the
// queued iterations', the settle's, the last iteration's.
constexpr uint32_t kSyncQueuedMax = 16, kSyncFlags = kSyncQueuedMax + 2;
constexpr uint32_t kSettledFlag = kSyncQueuedMax, kFinalFlag = kSyncQueuedMax + 1;
// 8: a single 4K SYN-v1 frame needs 5; round 5 queued 16 to stay clear of its
// one-lane settle (3.3 s when 4 were queued), but the round-6 parallel settle
// finishes a frame a few iterations short in ~10 ms, and each early-exiting
// launch past the fixpoint costs ~5 us (one 4K frame: resync 0.234 -> 0.186
// ms for 16 -> 8, 512 frames 1.41 -> 1.36; profiles/r06zm_syncq.log)
#ifndef NICE_SYNC_QUEUED
#define NICE_SYNC_QUEUED 8
#endif
constexpr uint32_t kSyncQueued = NICE_SYNC_QUEUED;
static_assert(kSyncQueued >= 1 && kSyncQueued <= kSyncQueuedMax, "queued sync iterations");
DecLayout dec_layout(uint32_t n_frames, uint64_t npx, const DecPlan& p) {
  const uint32_t max_chunks = p.max_chunks, n_ck = p.n_ck, ev_cap = p.ev_cap, subs = p.subs;
  DecLayout L{};
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
  L.o_tables = take((size_t)n_frames * sizeof(DecTables));
  L.o_dstart = take((size_t)n_frames * 8);
  L.o_entry = take((size_t)n_frames * max_chunks * 8);
  L.o_last = take((size_t)n_frames * max_chunks * 8);
  L.o_ck = take((size_t)n_frames * n_ck * max_chunks * 8);
  L.o_cpx = take((size_t)n_frames * max_chunks * 8);
  L.o_cstart = take((size_t)n_frames * max_chunks * 8);
  L.o_recs = take((size_t)n_frames * ((npx + 3) & ~3ull) * 4);
  L.o_changed = take(4 * kSyncFlags);
  L.o_fchanged = take((size_t)n_frames * 4);
  L.o_rowbuf = take(p.rowbuf);
  // first-pass pixel events (ev_cap per slice, 0: not kept)
  L.o_ev = take((size_t)n_frames * ((max_chunks + 63) & ~63u) * ev_cap * 4);
  L.o_evck = take(ev_cap ? (size_t)n_frames * n_ck * max_chunks * 4 : 0);
  L.o_evn = take(ev_cap ? (size_t)n_frames * max_chunks * 4 : 0);
  L.o_agree = take(ev_cap ? (size_t)n_frames * max_chunks * 4 : 0);
  L.o_items = take(ev_cap ? (size_t)n_frames * max_chunks * subs * 4 : 0);
  L.o_icount = take(ev_cap ? (size_t)n_frames * 4 : 0);
  // the re-parses' head events (hev_cap per slice, 0: not kept), laid out as the first pass's
  const uint32_t hev_cap = ev_cap ? p.hev_cap : 0u;
  L.o_hev = take((size_t)n_frames * ((max_chunks + 63) & ~63u) * hev_cap * 4);
  L.o_hevn = take(hev_cap ? (size_t)n_frames * max_chunks * 4 : 0);
  L.o_hevag = take(hev_cap ? (size_t)n_frames * max_chunks * 4 : 0);
  L.o_hand = take(p.hand);
  L.o_abort = take(p.abort_flags ? (size_t)n_frames * 4 : 0);
  L.total = o;
  return L;
}

// The plan's and the scratch layout's half of the kernel arguments.
void dec_args_scratch(DecArgs& a, const DecLayout& L, uint8_t* base, const DecPlan& P, uint64_t N) {
  a.tables = base + L.o_tables;
  a.data_start = (unsigned long long*)(base + L.o_dstart);
  const uint32_t max_chunks = P.max_chunks, cb = P.slice_bits;
  a.max_chunks = max_chunks;
  a.chunk_bits = cb;
  a.n_ck = P.n_ck;
  a.ck_bits = P.ck_bits;
  a.emit_blocks = (uint32_t)(((uint64_t)max_chunks * (cb / DEC_EMIT_BITS) + DEC_PARSE_THREADS - 1) / DEC_PARSE_THREADS);
  a.chunk_blocks = (max_chunks + DEC_PARSE_THREADS - 1) / DEC_PARSE_THREADS;
  a.chunk_px = (unsigned long long*)(base + L.o_cpx);
  a.chunk_start = (unsigned long long*)(base + L.o_cstart);
  a.entry = (unsigned long long*)(base + L.o_entry);
  a.last = (unsigned long long*)(base + L.o_last);
  a.ck = (unsigned long long*)(base + L.o_ck);
  a.recs = (uint32_t*)(base + L.o_recs);
  a.rec_stride = (N + 3) & ~3ull;
  a.seg = P.g.seg;
  a.nseg = P.g.nseg;
  a.rows_in_lds = P.g.in_lds ? 1u : 0u;
  a.parse_slow = opt_on(NICE_OPT_DEC_SLOW_PARSE) ? 1u : 0u;   // tests / A/B: the general parse only
  a.rowbuf = (uint32_t*)(base + L.o_rowbuf);
  if (P.ev_cap) {
    a.ev = (uint32_t*)(base + L.o_ev);
    a.ev_cap = P.ev_cap;
    a.ev_ck = (uint32_t*)(base + L.o_evck);
    a.ev_n = (uint32_t*)(base + L.o_evn);
    a.agree = (uint32_t*)(base + L.o_agree);
    a.head_items = (uint32_t*)(base + L.o_items);
    a.head_count = (uint32_t*)(base + L.o_icount);
    if (P.hev_cap) {
      a.hev = (uint32_t*)(base + L.o_hev);
      a.hev_cap = P.hev_cap;
      a.hev_n = (uint32_t*)(base + L.o_hevn);
      a.hev_ag = (uint32_t*)(base + L.o_hevag);
    }
  }
}

// One row-kernel launch of a plan (DecPlan::rows, or ::fallback with a.redo
// set): one block per frame; the split kernel one per strip, frames in chunks.
int launch_rows(const DecPlan& p, const DecLaunch& l, DecArgs& a, hipStream_t st) {
  void (*k)(DecArgs) = nullptr;
  switch (l.route) {
    case DEC_R_RECONSTRUCT: k = dec_reconstruct; break;
    case DEC_R_ROWS: k = dec_rows; break;
    case DEC_R_ROWS8: k = dec_rows8; break;
    case DEC_R_ROWS_WIDE: k = dec_rows_wide; break;
    case DEC_R_FLOW: k = dec_rows_flow; break;
    case DEC_R_SPLIT: k = dec_rows_split; break;
    default: return NICE_E_ARG;
  }
  if (l.lds > LDS_OPT_IN)
    NICE_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds));
  if (l.route != DEC_R_SPLIT) {
    hipLaunchKernelGGL(k, dim3(a.n_frames), dim3(l.threads), l.lds, st, a);
    return NICE_OK;
  }
  for (uint32_t f0 = 0; f0 < a.n_frames; f0 += p.split_frames) {
    a.split_f0 = f0;
    hipLaunchKernelGGL(k, dim3(std::min(p.split_frames, a.n_frames - f0) * p.strips), dim3(l.threads), l.lds, st, a);
  }
  a.split_f0 = 0;
  return NICE_OK;
}

// NICE_OPT_DEC_STATS: the kernels' counters (DecArgs::stats) and the sync
// flags to stderr, once the call's work on `st` is done
void dec_print_stats(hipStream_t st, const unsigned long long* dstats, const uint32_t* changed, uint32_t it_count,
                     uint32_t queued, const DecArgs& a) {
  unsigned long long h[128] = {0};
  (void)hipMemcpyAsync(h, dstats, 1024, hipMemcpyDeviceToHost, st);
  uint32_t chg[kSyncFlags] = {0};
  (void)hipMemcpyAsync(chg, changed, 4 * kSyncFlags, hipMemcpyDeviceToHost, st);
  // which parse each frame's tables allow (DecTables::fast, one byte a frame)
  // and frame 0's table plan: max_aob and lut_bits lie next to each other
  const uint8_t* tb = (const uint8_t*)a.tables;
  std::vector<uint8_t> tfast(a.n_frames, 0);
  uint8_t plan0[2 * N_STREAMS] = {0};
  static_assert(offsetof(DecTables, lut_bits) == offsetof(DecTables, max_aob) + N_STREAMS, "one copy for both");
  (void)hipMemcpy2DAsync(tfast.data(), 1, tb + offsetof(DecTables, fast), sizeof(DecTables), 1, a.n_frames,
                         hipMemcpyDeviceToHost, st);
  (void)hipMemcpyAsync(plan0, tb + offsetof(DecTables, max_aob), sizeof(plan0), hipMemcpyDeviceToHost, st);
  (void)hipStreamSynchronize(st);
  fprintf(stderr,
          "[nice dec stats] rows=%llu unconverged_segs=%llu tail_unknown_segs=%llu "
          "recomputed_px=%llu fixup_rounds=%llu sync_iters=%u seg=%u nseg=%u "
          "clk[load=%llu spec=%llu fix=%llu emit=%llu]\n",
          h[0], h[1], h[2], h[3], h[4], it_count, a.seg, a.nseg, h[5], h[6], h[7], h[8]);
  fprintf(stderr, "[nice dec stats] sync iterations that changed an entry:");
  for (uint32_t i = 0; i < kSyncFlags; ++i) fprintf(stderr, " %u", chg[i]);
  fprintf(stderr, " (queued %u, then settled, final)\n", queued);
  uint32_t n_fast = 0;
  for (uint8_t v : tfast) n_fast += v ? 1u : 0u;
  fprintf(stderr, "[nice dec stats] parse: frames=%u fast=%u slow_parse=%u frame0 max=", a.n_frames, n_fast,
          a.parse_slow);
  for (int s = 0; s < N_STREAMS; ++s) fprintf(stderr, "%s%u", s ? "," : "", (unsigned)plan0[s]);
  fprintf(stderr, " lut_bits=");
  for (int s = 0; s < N_STREAMS; ++s) fprintf(stderr, "%s%u", s ? "," : "", (unsigned)plan0[N_STREAMS + s]);
  fprintf(stderr, "\n");
  for (int w = 0; w < 4; ++w) {   // dec_rows_flow (-DNICE_FLOW_STATS builds): cycles per row by phase
    const unsigned long long* q = h + 64 + 8 * w;
    if (q[7])
      fprintf(stderr, "[nice flow stats] wave %d rows=%llu cyc/row: emit+decode=%.0f wait=%.0f ring=%.0f spec=%.0f "
              "fix=%.0f publish=%.0f rounds/row=%.2f\n", w, q[7], (double)q[0] / q[7], (double)q[1] / q[7],
              (double)q[2] / q[7], (double)q[3] / q[7], (double)q[4] / q[7], (double)q[5] / q[7],
              (double)q[6] / q[7]);
  }
  fprintf(stderr, "[nice dec stats] unknown segment tails: copies of an unknown %llu, narrowed %llu\n", h[24], h[25]);
  fprintf(stderr, "[nice dec stats] re-parse met previous parse at checkpoint:");
  for (int k = 0; k < 17; ++k) fprintf(stderr, " %d:%llu", k, h[32 + k]);
  fprintf(stderr, "\n");
  fprintf(stderr, "[nice dec stats] slice=%u emit waves=%llu wave_iters=%llu active_lane_iters=%llu fills=%llu\n",
          a.chunk_bits, h[20], h[16], h[17], h[18]);
  fprintf(stderr, "[nice dec stats] slices by first-pass meeting checkpoint: 0:%llu 1:%llu 2-4:%llu 5-16:%llu "
          "17-64:%llu 65+:%llu none:%llu overflow:%llu (ev_cap %u)\n",
          h[50], h[51], h[52], h[53], h[54], h[55], h[56], h[57], a.ev_cap);
  fprintf(stderr, "[nice dec stats] slice heads: none=%llu placed=%llu emitted=%llu whole_slice_emitted=%llu "
          "invariant_violations=%llu (hev_cap %u)\n", h[26], h[27], h[28], h[29], h[30], a.hev_cap);
  fprintf(stderr, "[nice dec stats] fix-up rounds per row: 0:%llu 1:%llu 2:%llu 3:%llu 4:%llu 5:%llu 6+:%llu\n",
          h[9], h[10], h[11], h[12], h[13], h[14], h[15]);
  if (h[61]) fprintf(stderr, "[nice dec stats] sync first pass: waves=%llu cycles/wave=%.0f refill cycles/wave=%.0f "
          "refills/wave=%.1f iterations/wave=%.1f active lane share=%.3f\n",
          h[61], h[61] ? (double)h[56] / h[61] : 0.0, h[61] ? (double)h[57] / h[61] : 0.0,
          h[61] ? (double)h[58] / h[61] : 0.0, h[61] ? (double)h[59] / h[61] : 0.0,
          h[59] ? (double)h[60] / (64.0 * h[59]) : 0.0);
}
}  // namespace

// ---- context-free host-buffer entry points --------------------------------
static std::mutex g_default_mu;
static nice_ctx* g_default = nullptr;

static int default_ctx(nice_ctx** out) {
  std::lock_guard<std::mutex> g(g_default_mu);
  if (!g_default) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    int rc = nice_ctx_create(dev, &g_default);
    if (rc) return rc;
  }
  *out = g_default;
  return NICE_OK;
}

int nice_encode(const uint8_t* px, size_t px_len, uint32_t w, uint32_t h, uint8_t channels,
                uint8_t channels_out, uint8_t* out, size_t out_cap, size_t* out_len) {
  if (!out || !out_len) return NICE_E_ARG;
  if (channels != 3 && channels != 4) return NICE_E_ARG;
  const uint64_t N = (uint64_t)w * h;
  if (px_len < N * channels || (N > 0 && !px)) return NICE_E_ARG;
  nice_ctx* ctx;
  int rc = default_ctx(&ctx);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  NICE_HIP(hipSetDevice(ctx->device));
  const size_t in_bytes = align_up((size_t)N * channels, 256);
  const size_t bound = align_up(nice_encode_bound(w, h), 256);
  if ((rc = ctx->host_px.grow(in_bytes + 256))) return rc;
  if ((rc = ctx->host_out.grow(bound))) return rc;
  if ((rc = ctx->dev_len.grow(256))) return rc;
  if (N) NICE_HIP(hipMemcpy(ctx->host_px.ptr, px, (size_t)N * channels, hipMemcpyHostToDevice));
  rc = nice_encode_batch_dev(ctx, nullptr, (const uint8_t*)ctx->host_px.ptr, in_bytes, 1, w, h,
                             channels, channels_out, (uint8_t*)ctx->host_out.ptr, bound,
                             (uint64_t*)ctx->dev_len.ptr);
  if (rc) return rc;
  uint64_t n = 0;
  NICE_HIP(hipMemcpy(&n, ctx->dev_len.ptr, 8, hipMemcpyDeviceToHost));
  if (n > out_cap) {
    *out_len = n;
    return NICE_E_CAPACITY;
  }
  NICE_HIP(hipMemcpy(out, ctx->host_out.ptr, n, hipMemcpyDeviceToHost));
  *out_len = n;
  return NICE_OK;
}


int nice_decode_batch_dev(nice_ctx* ctx, void* stream, const uint8_t* d_streams,
                          uint64_t stream_stride, const uint64_t* d_stream_len, uint32_t n_frames,
                          uint32_t w, uint32_t h, uint8_t out_channels, uint8_t* d_px,
                          uint64_t px_stride, uint32_t flags, int32_t* d_status) {
  return nice::decode_batch_impl(ctx, stream, d_streams, stream_stride, d_stream_len, nullptr, n_frames, w, h,
                                 out_channels, d_px, px_stride, flags, d_status);
}

int nice_decode_batch_dev_hl(nice_ctx* ctx, void* stream, const uint8_t* d_streams, uint64_t stream_stride,
                             const uint64_t* d_stream_len, const uint64_t* h_stream_len, uint32_t n_frames,
                             uint32_t w, uint32_t h, uint8_t out_channels, uint8_t* d_px, uint64_t px_stride,
                             uint32_t flags, int32_t* d_status) {
  if (n_frames && !h_stream_len) return NICE_E_ARG;
  return nice::decode_batch_impl(ctx, stream, d_streams, stream_stride, d_stream_len, h_stream_len, n_frames, w, h,
                                 out_channels, d_px, px_stride, flags, d_status);
}

// ---- packed stream batches -------------------------------------------------
uint64_t nice_packed_bound(uint32_t n_frames, uint32_t w, uint32_t h) {
  return (uint64_t)n_frames * align_up(nice_encode_bound(w, h), 16);
}

int nice_pack_streams_dev(nice_ctx* ctx, void* stream, const uint8_t* d_streams, uint64_t stream_stride,
                          const uint64_t* d_stream_len, uint32_t n_frames, uint8_t* d_packed, uint64_t packed_cap,
                          uint64_t* d_off, int32_t* d_status) {
  if (!ctx || !d_off || !d_status) return NICE_E_ARG;
  if (n_frames && (!d_streams || !d_stream_len)) return NICE_E_ARG;
  if (!d_packed && packed_cap) return NICE_E_ARG;
  if ((stream_stride & 3) || ((uintptr_t)d_streams & 3) || ((uintptr_t)d_packed & 15)) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  return nice::pack_streams_launch(stream, ctx->cus, d_streams, stream_stride, d_stream_len, n_frames, d_packed,
                                   packed_cap, d_off, d_status);
}

int nice_encode_batch_packed_dev(nice_ctx* ctx, void* stream, const uint8_t* d_px, uint64_t frame_stride,
                                 uint32_t n_frames, uint32_t w, uint32_t h, uint8_t channels, uint8_t channels_out,
                                 uint8_t* d_packed, uint64_t packed_cap, uint64_t* d_off, uint64_t* d_out_len,
                                 int32_t* d_status) {
  if (!ctx || !d_off || !d_out_len || !d_status) return NICE_E_ARG;
  if ((!d_packed && packed_cap) || ((uintptr_t)d_packed & 15)) return NICE_E_ARG;
  if ((uint64_t)w * h > (1ull << 30)) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  const uint64_t slot = packed_slot_bytes(w, h);
  int rc = ctx->pack.grow((size_t)n_frames * slot);
  if (rc) return rc;
  uint8_t* scratch = (uint8_t*)ctx->pack.ptr;
  if (n_frames) {
    rc = nice_encode_batch_dev(ctx, stream, d_px, frame_stride, n_frames, w, h, channels, channels_out, scratch, slot,
                               d_out_len);
    if (rc) return rc;
  } else if (channels != 3 && channels != 4) {
    return NICE_E_ARG;
  }
  return nice::pack_streams_launch(stream, ctx->cus, scratch, slot, d_out_len, n_frames, d_packed, packed_cap, d_off,
                                   d_status);
}

int nice_decode_packed_dev(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                           const uint64_t* d_off, const uint64_t* d_stream_len, const uint64_t* h_stream_len,
                           uint32_t n_frames, uint32_t w, uint32_t h, uint8_t out_channels, uint8_t* d_px,
                           uint64_t px_stride, uint32_t flags, int32_t* d_status) {
  if (!d_off) return NICE_E_ARG;
  return nice::decode_batch_impl(ctx, stream, d_packed, 0, d_stream_len, h_stream_len, n_frames, w, h, out_channels,
                                 d_px, px_stride, flags, d_status, d_off, packed_bytes);
}

}  // extern "C"

// h_stream_len: the lengths on the host when the caller has them (saves a
// device round trip), else nullptr.
int nice::decode_batch_impl(nice_ctx* ctx, void* stream, const uint8_t* d_streams, uint64_t stream_stride,
                            const uint64_t* d_stream_len, const uint64_t* h_stream_len, uint32_t n_frames,
                            uint32_t w, uint32_t h, uint8_t out_channels, uint8_t* d_px, uint64_t px_stride,
                            uint32_t flags, int32_t* d_status, const uint64_t* d_stream_off,
                            uint64_t packed_bytes) {
  if (!ctx || !d_streams || !d_stream_len || !d_status) return NICE_E_ARG;
  if (out_channels != 3 && out_channels != 4) return NICE_E_ARG;
  const bool packed = d_stream_off != nullptr;
  if (packed ? ((uintptr_t)d_streams & 15) != 0 : ((stream_stride & 3) || ((uintptr_t)d_streams & 3)))
    return NICE_E_ARG;
  const uint64_t N = (uint64_t)w * h;
  if (N > (1ull << 30)) return NICE_E_ARG;
  if (n_frames == 0) return NICE_OK;
  if (N > 0 && (!d_px || px_stride < N * out_channels)) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  ctx->split_frames = 0;
  NICE_HIP(hipMemsetAsync(d_status, 0, (size_t)n_frames * 4, st));
  // stream lengths bound the chunk grid
  std::vector<uint64_t> lens(n_frames);
  if (h_stream_len) {
    std::copy(h_stream_len, h_stream_len + n_frames, lens.begin());
  } else {
    NICE_HIP(hipMemcpyAsync(lens.data(), d_stream_len, (size_t)n_frames * 8, hipMemcpyDeviceToHost, st));
    NICE_HIP(hipStreamSynchronize(st));
  }
  uint64_t max_len = 0;
  for (uint64_t& l : lens) {
    // packed: a length the buffer cannot hold fails its frame on the device
    // (dec_tables), not the batch; it sizes no scratch
    if (!packed && l > stream_stride) return NICE_E_ARG;
    if (packed && l > packed_bytes) l = 0;
    max_len = l > max_len ? l : max_len;
  }
  const uint64_t D = FILE_HEADER_BYTES * 8 + TABLE_HEADER_BITS;
  uint64_t total_bits = 0;
  for (uint64_t l : lens) total_bits += l * 8 > D ? l * 8 - D : 0;
  auto opt = [](int id) { return DecOpt{opt_set(id), opt_val(id)}; };
  const DecOpts opts{opt(NICE_OPT_DEC_SLICE_BITS), opt(NICE_OPT_DEC_SINGLE_WAVE), opt(NICE_OPT_DEC_SEG),
                     opt(NICE_OPT_DEC_SPLIT),      opt(NICE_OPT_DEC_FLOW),        opt(NICE_OPT_DEC_NO_EVENTS),
                     opt(NICE_OPT_DEC_EV_CAP),     opt(NICE_OPT_DEC_HEV_CAP)};
  DecPlan P = plan_decode(DecShape{n_frames, w, h, ctx->cus, max_len, total_bits}, opts);
  ctx->last_dec_route = P.rows.route;
  ctx->last_dec_fallback = P.fallback.route;
  if (N > 0 && P.rows.route == DEC_R_NONE) return NICE_E_ARG;   // rows too wide for any row kernel
  DecLayout L = dec_layout(n_frames, N, P);
  int rc = ctx->dec.grow(L.total);
  if (rc && P.hev_cap) {   // the scratch does not fit: without the re-parses' head events
    (void)hipGetLastError();   // the failed allocation
    P.hev_cap = 0;
    L = dec_layout(n_frames, N, P);
    rc = ctx->dec.grow(L.total);
  }
  if (rc && P.ev_cap) {   // the scratch does not fit: without the first pass's events
    (void)hipGetLastError();   // the failed allocation
    P.ev_cap = 0;
    L = dec_layout(n_frames, N, P);
    rc = ctx->dec.grow(L.total);
  }
  if (rc) return rc;
  const uint32_t max_chunks = P.max_chunks;
  uint8_t* base = (uint8_t*)ctx->dec.ptr;
  DecArgs a{};
  a.streams = d_streams;
  a.stream_stride = stream_stride;
  a.stream_len = (const unsigned long long*)d_stream_len;
  a.stream_off = (const unsigned long long*)d_stream_off;
  a.packed_bytes = packed_bytes;
  a.n_frames = n_frames;
  a.W = w;
  a.H = h;
  a.out_channels = out_channels;
  a.flags = flags;
  a.px_out = d_px;
  a.px_stride = px_stride;
  a.status = d_status;
  dec_args_scratch(a, L, base, P, N);
  uint32_t* changed = (uint32_t*)(base + L.o_changed);

  PhaseTimer& tm = ctx->timer;
  tm.begin(NICE_PH_DEC_TABLES, st);
  hipLaunchKernelGGL(dec_tables, dim3(n_frames), dim3(256), 0, st, a);
  tm.end(st);
  if (N == 0) {
    NICE_HIP(hipGetLastError());
    return NICE_OK;
  }
  const bool want_stats = opt_on(NICE_OPT_DEC_STATS);
  unsigned long long* dstats = nullptr;
  if (want_stats && hipMalloc(&dstats, 1024) == hipSuccess) {
    (void)hipMemsetAsync(dstats, 0, 1024, st);
    a.stats = dstats;
  }
  hipLaunchKernelGGL(dec_init_entries, dim3((max_chunks + 255) / 256 < 64 ? (max_chunks + 255) / 256 : 64, n_frames),
                     dim3(256), 0, st, a);
  const dim3 cgrid(n_frames * a.chunk_blocks);
  // Jacobi iteration of the chunk entry states to the fixpoint, all on the
  // device: queued iterations (each returns at once if the previous one changed
  // nothing), the sequential settle of frames still changing after the last
  // one, and one more iteration for the slices the settle moved
  uint32_t it_count = 0;
  uint32_t queued = std::min(kSyncQueued, max_chunks + 1);
  if (opt_set(NICE_OPT_DEC_SYNC_QUEUED)) {   // tests: fewer queued iterations
    const uint32_t v = (uint32_t)opt_val(NICE_OPT_DEC_SYNC_QUEUED);
    if (v >= 1 && v <= kSyncQueuedMax) queued = std::min(v, max_chunks + 1);
  }
  uint32_t* fchanged = (uint32_t*)(base + L.o_fchanged);
  NICE_HIP(hipMemsetAsync(changed, 0, 4 * kSyncFlags, st));
  NICE_HIP(hipMemsetAsync(fchanged, 0, (size_t)n_frames * 4, st));
  for (uint32_t it = 0; it < queued; ++it, ++it_count) {
    tm.begin(it ? NICE_PH_DEC_RESYNC : NICE_PH_DEC_SYNC, st);
    hipLaunchKernelGGL(dec_sync, cgrid, dim3(DEC_PARSE_THREADS), 0, st, a, changed + it, it ? changed + it - 1 : nullptr,
                       it + 1 == queued ? fchanged : nullptr);
    tm.end(st);
  }
  tm.begin(NICE_PH_DEC_RESYNC, st);
  hipLaunchKernelGGL(dec_sync_settle, dim3(n_frames), dim3(SETTLE_THREADS), 0, st, a, changed + queued - 1, fchanged,
                     changed + kSettledFlag);
  // the last iteration, for the slices the settle moved: it must change no
  // entry; a frame where it does (a settle that disagreed with dec_sync) is
  // failed by dec_scan instead of decoded from a non-fixpoint
  NICE_HIP(hipMemsetAsync(fchanged, 0, (size_t)n_frames * 4, st));
  hipLaunchKernelGGL(dec_sync, cgrid, dim3(DEC_PARSE_THREADS), 0, st, a, changed + kFinalFlag,
                     changed + kSettledFlag, fchanged);
  tm.end(st);
  // the last sync iteration (no entry changed) already produced chunk_px
  tm.begin(NICE_PH_DEC_SCAN, st);
  a.unsettled = fchanged;
  hipLaunchKernelGGL(dec_scan, dim3(n_frames), dim3(1024), 0, st, a);
  a.unsettled = nullptr;
  // strict: the reads where the reference's refill loop would wrap (frames
  // whose tables are all <= 25 bits return at once)
  if (flags & NICE_DEC_STRICT_REFERENCE) hipLaunchKernelGGL(dec_strict_refill, cgrid, dim3(DEC_PARSE_THREADS), 0, st, a);
  tm.end(st);
  tm.begin(NICE_PH_DEC_EMIT, st);
  if (a.ev) hipLaunchKernelGGL(dec_heads, dim3(n_frames), dim3(1024), 0, st, a);
  {
    // run pixels: slots without this call's tag.  Clear (tag 0) only when the
    // region moved or resized (other data may have held it) or the tags wrap.
    const uint64_t words = (uint64_t)n_frames * a.rec_stride;
    if (a.recs != ctx->rec_region || words != ctx->rec_words || ctx->dec.gen != ctx->rec_gen ||
        ctx->rec_epoch >= 15u || opt_on(NICE_OPT_DEC_REC_CLEAR)) {
      NICE_HIP(hipMemsetAsync(a.recs, 0, words * 4, st));
      ctx->rec_region = a.recs;
      ctx->rec_words = words;
      ctx->rec_gen = ctx->dec.gen;
      ctx->rec_epoch = 0;
    }
    a.rec_tag = ++ctx->rec_epoch;
  }
  hipLaunchKernelGGL(dec_emit, dim3(n_frames * a.emit_blocks), dim3(DEC_PARSE_THREADS), 0, st, a);
  tm.end(st);
  if (a.ev) {
    tm.begin(NICE_PH_DEC_PLACE, st);
    hipLaunchKernelGGL(dec_place, dim3((max_chunks + DEC_PLACE_WAVES - 1) / DEC_PLACE_WAVES, n_frames), dim3(64 * DEC_PLACE_WAVES), 0, st, a);
    tm.end(st);
  }
  tm.begin(NICE_PH_DEC_RECON, st);
  if (P.abort_flags) {
    a.hand_abort = (uint32_t*)(base + L.o_abort);
    NICE_HIP(hipMemsetAsync(a.hand_abort, 0, (size_t)n_frames * 4, st));
    ctx->split_abort = a.hand_abort;
    ctx->split_frames = n_frames;
  }
  if (P.rows.route == DEC_R_SPLIT) {
    a.strips = P.strips;
    a.hand = (unsigned long long*)(base + L.o_hand);
    NICE_HIP(hipMemsetAsync(a.hand, 0, P.hand, st));
    a.test_absent_strip = ctx->test_split_absent;
  } else if (P.rows.route == DEC_R_FLOW) {
    a.flow_k = P.flow_k;
    a.flow_ring = P.flow_ring;
    a.test_absent_strip = opt_on(NICE_OPT_TEST_FLOW_ABSENT) ? 1u : 0u;
  }
  if ((rc = launch_rows(P, P.rows, a, st))) return rc;
  if (P.fallback.route != DEC_R_NONE) {   // its blocks return at once for every frame not marked SPLIT_REDO
    a.test_absent_strip = 0;
    a.redo = 1;
    if ((rc = launch_rows(P, P.fallback, a, st))) return rc;
  }
  tm.end(st);
  if (dstats) {
    dec_print_stats(st, dstats, changed, it_count, queued, a);
    (void)hipFree(dstats);
  }
  NICE_HIP(hipGetLastError());
  return NICE_OK;
}

extern "C" {

// ---- tiled images ----------------------------------------------------------
int nice_tile_grid(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t* nx, uint32_t* ny) {
  if (!nx || !ny) return NICE_E_ARG;
  return nice::tile_grid(w, h, tile_w, tile_h, nx, ny);
}

uint64_t nice_tiled_bound(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h) {
  uint32_t nx, ny;
  if (nice_tile_grid(w, h, tile_w, tile_h, &nx, &ny)) return 0;
  return nice_packed_bound(nx * ny, tile_w, tile_h);
}

int nice_tile_select(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t x0, uint32_t y0, uint32_t rw,
                     uint32_t rh, uint32_t* tx0, uint32_t* ty0, uint32_t* tx1, uint32_t* ty1) {
  uint32_t nx, ny;
  TileRange r;
  if (!tx0 || !ty0 || !tx1 || !ty1) return NICE_E_ARG;
  int rc = nice::tile_select(w, h, tile_w, tile_h, x0, y0, rw, rh, &nx, &ny, &r);
  if (rc) return rc;
  *tx0 = r.tx0;
  *ty0 = r.ty0;
  *tx1 = r.tx1;
  *ty1 = r.ty1;
  return NICE_OK;
}

int nice_tiles_split_dev(nice_ctx* ctx, void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w, uint32_t h,
                         uint8_t channels, uint32_t tile_w, uint32_t tile_h, uint8_t* d_tiles, uint64_t tile_stride) {
  if (!ctx || !d_img || !d_tiles || (channels != 3 && channels != 4)) return NICE_E_ARG;
  uint32_t nx, ny;
  int rc = nice_tile_grid(w, h, tile_w, tile_h, &nx, &ny);
  if (rc) return rc;
  if (row_pitch < (uint64_t)w * channels || tile_stride < (uint64_t)tile_w * tile_h * channels) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  return nice::tiles_split_launch(stream, d_img, row_pitch, w, h, channels, tile_w, tile_h, nx, ny, d_tiles,
                                  tile_stride);
}

int nice_tiles_merge_dev(nice_ctx* ctx, void* stream, const uint8_t* d_tiles, uint64_t tile_stride,
                         const uint32_t* d_tile_idx, uint32_t n_slots, uint8_t tile_channels, uint32_t w, uint32_t h,
                         uint32_t tile_w, uint32_t tile_h, uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh,
                         uint8_t out_channels, uint8_t alpha, uint8_t* d_out, uint64_t out_pitch) {
  if (!ctx || !d_out) return NICE_E_ARG;
  if ((tile_channels != 3 && tile_channels != 4) || (out_channels != 3 && out_channels != 4)) return NICE_E_ARG;
  uint32_t nx, ny;
  TileRange r;
  int rc = nice::tile_select(w, h, tile_w, tile_h, x0, y0, rw, rh, &nx, &ny, &r);
  if (rc) return rc;
  if (out_pitch < (uint64_t)rw * out_channels) return NICE_E_ARG;
  if (n_slots == 0) return NICE_OK;
  if (!d_tiles || !d_tile_idx || tile_stride < (uint64_t)tile_w * tile_h * tile_channels) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  return nice::tiles_merge_launch(stream, d_tiles, tile_stride, nullptr, d_tile_idx, nullptr, n_slots, w, h, tile_w,
                                  tile_h, nx, ny, x0, y0, rw, rh, tile_channels, out_channels, alpha, d_out, out_pitch);
}

namespace {
// The scratch of a verified encode of n dense tiles: the tiles, their decode,
// the strided stream slots, and tab_bytes of small tables that begin with the
// verify decode's statuses (4 bytes a tile).
struct TileEncScratch { uint64_t tile_stride, slot; };
int tile_enc_scratch(nice_ctx* ctx, uint32_t n, uint32_t tile_w, uint32_t tile_h, uint8_t channels, size_t tab_bytes,
                     TileEncScratch& s) {
  int rc;
  s.tile_stride = align_up((size_t)tile_w * tile_h * channels, 16);
  s.slot = packed_slot_bytes(tile_w, tile_h);
  if ((rc = ctx->tiles.grow((size_t)n * s.tile_stride))) return rc;
  if ((rc = ctx->tile_dec.grow((size_t)n * s.tile_stride))) return rc;
  if ((rc = ctx->pack.grow((size_t)n * s.slot))) return rc;
  return ctx->tile_tab.grow(tab_bytes);
}

// The n dense tiles in ctx->tiles to a packed batch, always lossless: encode,
// decode again, compare, store raw what the codec did not return, pack.
int encode_tiles_verified(nice_ctx* ctx, void* stream, uint32_t n, uint32_t tile_w, uint32_t tile_h, uint8_t channels,
                          uint8_t channels_out, const TileEncScratch& s, uint8_t* d_packed, uint64_t packed_cap,
                          uint64_t* d_off, uint64_t* d_len, uint8_t* d_kind, int32_t* d_status) {
  int rc;
  const uint32_t npx = tile_w * tile_h;
  uint8_t* tiles = (uint8_t*)ctx->tiles.ptr;
  uint8_t* back = (uint8_t*)ctx->tile_dec.ptr;
  uint8_t* slots = (uint8_t*)ctx->pack.ptr;
  int32_t* dec_status = (int32_t*)ctx->tile_tab.ptr;
  if ((rc = nice_encode_batch_dev(ctx, stream, tiles, s.tile_stride, n, tile_w, tile_h, channels, channels_out, slots,
                                  s.slot, d_len)))
    return rc;
  // verify: a table header the format cannot carry (SURVEY.md Appendix A.5,
  // DESIGN.md "Tiled images") shows as a failed or a different decode
  if ((rc = nice::decode_batch_impl(ctx, stream, slots, s.slot, d_len, nullptr, n, tile_w, tile_h, channels, back,
                                    s.tile_stride, NICE_DEC_TOLERANT_HEADER, dec_status)))
    return rc;
  if ((rc = nice::tiles_compare_launch(stream, tiles, s.tile_stride, back, s.tile_stride, channels, n, npx, dec_status,
                                       d_kind)))
    return rc;
  if ((rc = nice::tiles_store_raw_launch(stream, tiles, s.tile_stride, channels, n, npx, d_kind, slots, s.slot, d_len)))
    return rc;
  return nice::pack_streams_launch(stream, ctx->cus, slots, s.slot, d_len, n, d_packed, packed_cap, d_off, d_status);
}

// A slot plan with its table, and where both went on the device: the callers'
// window descriptors at `head`, the columns the merges read, the nc coded slots
// decoded `stride` apart at `dec` with their statuses at c_st; ns: the raw
// (colour) or the accepted (alpha) slots.  The host copies live here because
// the uploads and the batch decode read them.
struct DevSlots {
  SlotPlan plan;
  SlotTable tab;
  uint32_t nc = 0, ns = 0;
  const uint8_t *head = nullptr, *dec = nullptr, *s_kind = nullptr;
  uint64_t stride = 0;
  const int32_t* c_st = nullptr;
  const uint32_t *c_idx = nullptr, *c_win = nullptr, *s_idx = nullptr, *s_win = nullptr;
  const uint64_t* s_src = nullptr;
};

// What every tiled and set decode does with d.plan, up to its merges: one
// upload of `head` (head_bytes, a multiple of 8) and the plan's columns, the
// initial statuses, the batch decode of the coded slots (w x h at `channels`
// bytes per pixel) from their offsets in the packed batch, and the scatter of
// its statuses into d_status.
int decode_planned_slots(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes, const void* head,
                         size_t head_bytes, uint32_t w, uint32_t h, uint8_t channels, uint32_t flags, int32_t* d_status,
                         DevSlots& d) {
  int rc;
  hipStream_t st = (hipStream_t)stream;
  const SlotPlan& p = d.plan;
  const SlotTable& t = d.tab;
  pack_slot_table(p, head, head_bytes, d.tab);
  d.nc = (uint32_t)p.c_off.size();
  d.ns = (uint32_t)p.s_idx.size();
  d.stride = align_up((size_t)w * h * channels, 16);
  if ((rc = ctx->tile_tab.grow(std::max<size_t>(t.bytes, 16)))) return rc;
  if (d.nc && (rc = ctx->tile_dec.grow((size_t)d.nc * d.stride))) return rc;
  uint8_t* dt = (uint8_t*)ctx->tile_tab.ptr;
  int32_t* cst = (int32_t*)(dt + t.c_st);
  d.head = dt;
  d.dec = (const uint8_t*)ctx->tile_dec.ptr;
  d.c_st = cst;
  d.c_idx = (const uint32_t*)(dt + t.c_idx);
  d.c_win = (const uint32_t*)(dt + t.c_win);
  d.s_src = (const uint64_t*)(dt + t.s_src);
  d.s_idx = (const uint32_t*)(dt + t.s_idx);
  d.s_win = (const uint32_t*)(dt + t.s_win);
  d.s_kind = dt + t.s_kind;
  if (t.c_st) NICE_HIP(hipMemcpyAsync(dt, t.host.data(), t.c_st, hipMemcpyHostToDevice, st));
  NICE_HIP(hipMemcpyAsync(d_status, p.init.data(), 4ull * p.init.size(), hipMemcpyHostToDevice, st));
  if (!d.nc) return NICE_OK;
  if ((rc = nice::decode_batch_impl(ctx, stream, d_packed, 0, (const uint64_t*)(dt + t.c_len), p.c_len.data(), d.nc, w, h,
                                    channels, (uint8_t*)ctx->tile_dec.ptr, d.stride, flags, cst,
                                    (const uint64_t*)(dt + t.c_off), packed_bytes)))
    return rc;
  return nice::tiles_scatter_status_launch(stream, cst, (const uint32_t*)(dt + t.c_pos), d.nc, d_status);
}
}  // namespace

int nice_encode_tiled_dev(nice_ctx* ctx, void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w, uint32_t h,
                          uint8_t channels, uint8_t channels_out, uint32_t tile_w, uint32_t tile_h, uint8_t* d_packed,
                          uint64_t packed_cap, uint64_t* d_off, uint64_t* d_len, uint8_t* d_kind, int32_t* d_status) {
  if (!ctx || !d_img || !d_off || !d_len || !d_kind || !d_status) return NICE_E_ARG;
  if (channels != 3 && channels != 4) return NICE_E_ARG;
  if ((!d_packed && packed_cap) || ((uintptr_t)d_packed & 15)) return NICE_E_ARG;
  uint32_t nx, ny;
  int rc = nice_tile_grid(w, h, tile_w, tile_h, &nx, &ny);
  if (rc) return rc;
  if (row_pitch < (uint64_t)w * channels) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  const uint32_t n = nx * ny;
  TileEncScratch s;
  if ((rc = tile_enc_scratch(ctx, n, tile_w, tile_h, channels, (size_t)n * 4, s))) return rc;
  if ((rc = nice::tiles_split_launch(stream, d_img, row_pitch, w, h, channels, tile_w, tile_h, nx, ny,
                                     (uint8_t*)ctx->tiles.ptr, s.tile_stride)))
    return rc;
  return encode_tiles_verified(ctx, stream, n, tile_w, tile_h, channels, channels_out, s, d_packed, packed_cap, d_off,
                               d_len, d_kind, d_status);
}

int nice_decode_tiled_dev(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                          const uint64_t* h_off, const uint64_t* h_len, const uint8_t* h_kind, uint32_t w, uint32_t h,
                          uint32_t tile_w, uint32_t tile_h, uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh,
                          uint8_t out_channels, uint8_t* d_out, uint64_t out_pitch, uint32_t flags, int32_t* d_status) {
  if (!ctx || !d_packed || !h_off || !h_len || !h_kind || !d_out || !d_status) return NICE_E_ARG;
  if (out_channels != 3 && out_channels != 4) return NICE_E_ARG;
  if ((flags & NICE_DEC_STRICT_REFERENCE) || ((uintptr_t)d_packed & 15)) return NICE_E_ARG;
  uint32_t nx, ny;
  TileRange r;
  int rc = nice::tile_select(w, h, tile_w, tile_h, x0, y0, rw, rh, &nx, &ny, &r);
  if (rc) return rc;
  if (out_pitch < (uint64_t)rw * out_channels) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  // the one-image set with one window; a tile refused by the plan keeps its status and is not touched
  const uint32_t first[2] = {0, nx * ny}, win[5] = {0, x0, y0, rw, rh};
  DevSlots d;
  plan_colour_slots(SlotTables{h_off, h_len, h_kind, nullptr, packed_bytes},
                    SlotWindows{tile_w, tile_h, first, &nx, win, 1, false}, d.plan);
  ctx->last_tiled_coded = d.plan.by_kind[0];
  ctx->last_tiled_raw = d.plan.by_kind[1];
  if ((rc = decode_planned_slots(ctx, stream, d_packed, packed_bytes, nullptr, 0, tile_w, tile_h, out_channels,
                                 (flags & NICE_DEC_ALPHA_FILL_FF) | NICE_DEC_TOLERANT_HEADER, d_status, d)))
    return rc;
  if (d.nc) {
    if ((rc = nice::tiles_merge_launch(stream, d.dec, d.stride, nullptr, d.c_idx, d.c_st, d.nc, w, h, tile_w, tile_h, nx,
                                       ny, x0, y0, rw, rh, out_channels, out_channels, 0, d_out, out_pitch)))
      return rc;
  }
  if (d.ns) {
    const uint32_t fill = (flags & NICE_DEC_ALPHA_FILL_FF) ? 255u : 0u;
    if ((rc = nice::tiles_merge_launch(stream, d_packed, 0, d.s_src, d.s_idx, nullptr, d.ns, w, h, tile_w, tile_h, nx, ny,
                                       x0, y0, rw, rh, 3, out_channels, fill, d_out, out_pitch)))
      return rc;
  }
  return NICE_OK;
}

// ---- tiled images: the alpha batch ------------------------------------------
uint32_t nice_tile_alpha_width(uint32_t tile_w) { return (uint32_t)(((uint64_t)tile_w + 2) / 3); }

// a slot of the alpha encode's strided scratch: the stream or the raw plane
static uint64_t alpha_slot_bytes(uint32_t tile_w, uint32_t tile_h) {
  return std::max<uint64_t>(packed_slot_bytes(nice_tile_alpha_width(tile_w), tile_h),
                            align_up((size_t)tile_w * tile_h, 256));
}

uint64_t nice_tiled_alpha_bound(uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h) {
  uint32_t nx, ny;
  if (nice_tile_grid(w, h, tile_w, tile_h, &nx, &ny)) return 0;
  const uint64_t per = std::max<uint64_t>(nice_encode_bound(nice_tile_alpha_width(tile_w), tile_h),
                                          (uint64_t)tile_w * tile_h);
  return (uint64_t)nx * ny * align_up(per, 16);
}

int nice_tiles_alpha_range_dev(nice_ctx* ctx, void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w,
                               uint32_t h, uint32_t tile_w, uint32_t tile_h, uint32_t* d_lo, uint32_t* d_hi) {
  if (!ctx || !d_img || !d_lo || !d_hi) return NICE_E_ARG;
  uint32_t nx, ny;
  int rc = nice_tile_grid(w, h, tile_w, tile_h, &nx, &ny);
  if (rc) return rc;
  if (row_pitch < 4ull * w) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  return nice::alpha_range_launch(stream, d_img, row_pitch, w, h, tile_w, tile_h, nx, ny, d_lo, d_hi);
}

namespace {
// The small tables of an alpha encode of n tiles, sized for every tile coded,
// at the start of ctx->tile_tab: the stream lengths, the ranges, the list of
// coded tiles, their decode statuses and verdicts; `end` is 16-byte aligned.
// The host arrays live here because the copies to the device read them.
struct AlphaEnc {
  uint32_t n = 0, m = 0;   // tiles; tiles that are not constant
  size_t o_mlen = 0, o_lo = 0, o_hi = 0, o_list = 0, o_st = 0, o_vk = 0, end = 0;
  uint64_t slot = 0, trip_stride = 0;
  std::vector<uint32_t> list;
  std::vector<uint8_t> kind, val;
  explicit AlphaEnc(uint32_t n_tiles) : n(n_tiles) {
    o_lo = o_mlen + 8ull * n;
    o_hi = o_lo + 4ull * n;
    o_list = o_hi + 4ull * n;
    o_st = o_list + 4ull * n;
    o_vk = o_st + 4ull * n;
    end = align_up(o_vk + n, 16);
  }
};

// After the range launch: the first wait (the ranges say which tiles are coded
// at all), then d_akind, d_aval, zero lengths, and for m > 0 the scratch of
// the coded tiles and their list on the device, ready for the gather.
int alpha_encode_classify(nice_ctx* ctx, hipStream_t st, uint32_t tile_w, uint32_t tile_h, AlphaEnc& a, uint64_t* d_alen,
                          uint8_t* d_akind, uint8_t* d_aval) {
  int rc;
  const uint32_t n = a.n;
  uint8_t* dt = (uint8_t*)ctx->tile_tab.ptr;
  std::vector<uint32_t> range(2ull * n);
  NICE_HIP(hipMemcpyAsync(range.data(), dt + a.o_lo, 8ull * n, hipMemcpyDeviceToHost, st));
  NICE_HIP(hipStreamSynchronize(st));
  a.kind.resize(n);
  a.val.resize(n);
  for (uint32_t t = 0; t < n; ++t) {
    const bool flat = range[t] == range[n + t];
    a.kind[t] = flat ? 2 : 0;
    a.val[t] = flat ? (uint8_t)range[t] : 0;
    if (!flat) a.list.push_back(t);
  }
  a.m = (uint32_t)a.list.size();
  NICE_HIP(hipMemcpyAsync(d_akind, a.kind.data(), n, hipMemcpyHostToDevice, st));
  NICE_HIP(hipMemcpyAsync(d_aval, a.val.data(), n, hipMemcpyHostToDevice, st));
  NICE_HIP(hipMemsetAsync(d_alen, 0, 8ull * n, st));
  a.slot = alpha_slot_bytes(tile_w, tile_h);
  a.trip_stride = align_up((size_t)nice_tile_alpha_width(tile_w) * 3 * tile_h, 16);
  if (!a.m) return NICE_OK;
  if ((rc = ctx->tiles.grow((size_t)a.m * a.trip_stride))) return rc;
  if ((rc = ctx->tile_dec.grow((size_t)a.m * a.trip_stride))) return rc;
  if ((rc = ctx->pack.grow((size_t)a.m * a.slot))) return rc;
  NICE_HIP(hipMemcpyAsync(dt + a.o_list, a.list.data(), 4ull * a.m, hipMemcpyHostToDevice, st));
  return NICE_OK;
}

// After the gather launch: the m triplet images in ctx->tiles to streams or
// raw planes (encode, decode again, compare, store), the offsets of all n
// tiles, and the streams and planes to their places.
int alpha_encode_finish(nice_ctx* ctx, void* stream, uint32_t tile_w, uint32_t tile_h, const AlphaEnc& a,
                        uint8_t* d_apacked, uint64_t apacked_cap, uint64_t* d_aoff, uint64_t* d_alen, uint8_t* d_akind,
                        int32_t* d_status) {
  int rc;
  const uint32_t m = a.m, aw = nice_tile_alpha_width(tile_w);
  uint8_t* dt = (uint8_t*)ctx->tile_tab.ptr;
  uint8_t* slots = (uint8_t*)ctx->pack.ptr;
  uint32_t* d_list = (uint32_t*)(dt + a.o_list);
  uint64_t* mlen = (uint64_t*)(dt + a.o_mlen);
  if (m) {
    uint8_t* trip = (uint8_t*)ctx->tiles.ptr;
    uint8_t* back = (uint8_t*)ctx->tile_dec.ptr;
    int32_t* dec_status = (int32_t*)(dt + a.o_st);
    uint8_t* vk = dt + a.o_vk;
    if ((rc = nice_encode_batch_dev(ctx, stream, trip, a.trip_stride, m, aw, tile_h, 3, 3, slots, a.slot, mlen)))
      return rc;
    // second wait: the stream lengths size the verify decode, as in encode_tiles_verified
    if ((rc = nice::decode_batch_impl(ctx, stream, slots, a.slot, mlen, nullptr, m, aw, tile_h, 3, back, a.trip_stride,
                                      NICE_DEC_TOLERANT_HEADER, dec_status)))
      return rc;
    if ((rc = nice::tiles_compare_launch(stream, trip, a.trip_stride, back, a.trip_stride, 3, m, aw * tile_h, dec_status,
                                         vk)))
      return rc;
    if ((rc = nice::alpha_store_launch(stream, trip, a.trip_stride, tile_w, tile_h, d_list, m, vk, mlen, slots, a.slot,
                                       d_akind, d_alen)))
      return rc;
  }
  if ((rc = nice::pack_offsets_launch(stream, a.slot, d_alen, a.n, apacked_cap, d_aoff, d_status))) return rc;
  return m ? nice::alpha_pack_launch(stream, slots, a.slot, mlen, d_list, m, d_aoff, d_apacked, apacked_cap) : NICE_OK;
}
}  // namespace

int nice_encode_tiled_alpha_dev(nice_ctx* ctx, void* stream, const uint8_t* d_img, uint64_t row_pitch, uint32_t w,
                                uint32_t h, uint32_t tile_w, uint32_t tile_h, uint8_t* d_apacked, uint64_t apacked_cap,
                                uint64_t* d_aoff, uint64_t* d_alen, uint8_t* d_akind, uint8_t* d_aval,
                                int32_t* d_status) {
  if (!ctx || !d_img || !d_aoff || !d_alen || !d_akind || !d_aval || !d_status) return NICE_E_ARG;
  if ((!d_apacked && apacked_cap) || ((uintptr_t)d_apacked & 15)) return NICE_E_ARG;
  uint32_t nx, ny;
  int rc = nice_tile_grid(w, h, tile_w, tile_h, &nx, &ny);
  if (rc) return rc;
  if (row_pitch < 4ull * w) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  AlphaEnc a(nx * ny);
  if ((rc = ctx->tile_tab.grow(a.end))) return rc;
  uint8_t* dt = (uint8_t*)ctx->tile_tab.ptr;
  if ((rc = nice::alpha_range_launch(stream, d_img, row_pitch, w, h, tile_w, tile_h, nx, ny, (uint32_t*)(dt + a.o_lo),
                                     (uint32_t*)(dt + a.o_hi))))
    return rc;
  if ((rc = alpha_encode_classify(ctx, (hipStream_t)stream, tile_w, tile_h, a, d_alen, d_akind, d_aval))) return rc;
  if (a.m && (rc = nice::alpha_gather_launch(stream, d_img, row_pitch, w, h, tile_w, tile_h, nx,
                                             (const uint32_t*)(dt + a.o_list), a.m, (uint8_t*)ctx->tiles.ptr,
                                             a.trip_stride)))
    return rc;
  return alpha_encode_finish(ctx, stream, tile_w, tile_h, a, d_apacked, apacked_cap, d_aoff, d_alen, d_akind, d_status);
}

int nice_decode_tiled_alpha_dev(nice_ctx* ctx, void* stream, const uint8_t* d_apacked, uint64_t apacked_bytes,
                                const uint64_t* h_aoff, const uint64_t* h_alen, const uint8_t* h_akind,
                                const uint8_t* h_aval, uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h,
                                uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh, uint8_t* d_out, uint64_t out_pitch,
                                int32_t* d_status) {
  if (!ctx || !h_aoff || !h_alen || !h_akind || !h_aval || !d_out || !d_status) return NICE_E_ARG;
  if ((!d_apacked && apacked_bytes) || ((uintptr_t)d_apacked & 15)) return NICE_E_ARG;
  uint32_t nx, ny;
  TileRange r;
  int rc = nice::tile_select(w, h, tile_w, tile_h, x0, y0, rw, rh, &nx, &ny, &r);
  if (rc) return rc;
  if (out_pitch < 4ull * rw) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  // the coded tiles to decode, and every accepted tile to merge with its source
  const uint32_t first[2] = {0, nx * ny}, win[5] = {0, x0, y0, rw, rh};
  DevSlots d;
  plan_alpha_slots(SlotTables{h_aoff, h_alen, h_akind, h_aval, apacked_bytes},
                   SlotWindows{tile_w, tile_h, first, &nx, win, 1, false}, d.plan);
  if ((rc = decode_planned_slots(ctx, stream, d_apacked, apacked_bytes, nullptr, 0, nice_tile_alpha_width(tile_w), tile_h,
                                 3, NICE_DEC_TOLERANT_HEADER, d_status, d)))
    return rc;
  return nice::alpha_merge_launch(stream, d.dec, d.stride, d.c_st, d_apacked, d.s_src, d.s_kind, d.s_idx, d.ns, w, h,
                                  tile_w, tile_h, nx, x0, y0, rw, rh, d_out, out_pitch);
}

// ---- image sets --------------------------------------------------------------
int nice_set_grid(const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                  uint32_t* first) {
  return nice::set_grid(h_w, h_h, K, tile_w, tile_h, first, nullptr);
}

uint64_t nice_set_bound(const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h) {
  std::vector<uint32_t> first((size_t)K + 1);
  if (nice_set_grid(h_w, h_h, K, tile_w, tile_h, first.data())) return 0;
  return nice_packed_bound(first[K], tile_w, tile_h);
}

int nice_set_select(const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                    const uint32_t* h_win, uint32_t M, uint32_t* slot_first) {
  std::vector<uint32_t> first, nx;
  return nice::set_select(h_w, h_h, K, tile_w, tile_h, h_win, M, first, nx, slot_first);
}

namespace {
// The image descriptors of a set (checked: pointers, pitches); NICE_E_ARG otherwise.
int set_image_table(const uint8_t* const* h_img, const uint64_t* h_pitch, const uint32_t* h_w, const uint32_t* h_h,
                    uint32_t K, uint32_t channels, uint32_t tile_w, const uint32_t* first, std::vector<SetImage>& tab) {
  if (!h_img || !h_pitch) return NICE_E_ARG;
  tab.resize(K);
  for (uint32_t i = 0; i < K; ++i) {
    if (!h_img[i] || h_pitch[i] < (uint64_t)h_w[i] * channels) return NICE_E_ARG;
    tab[i] = SetImage{h_img[i], h_pitch[i], h_w[i], h_h[i], (h_w[i] + tile_w - 1) / tile_w, first[i],
                      nice::set_image_mode(h_img[i], h_pitch[i]), 0};
  }
  return NICE_OK;
}

// The window descriptors of M windows {image, x0, y0, rw, rh} (checked as by
// nice_set_select, plus pointers and pitches).
int set_window_table(const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                     const uint32_t* h_win, uint8_t* const* h_out, const uint64_t* h_out_pitch, uint32_t M,
                     uint32_t out_channels, std::vector<SetWindow>& tab) {
  if (!h_out || !h_out_pitch) return NICE_E_ARG;
  tab.resize(M);
  for (uint32_t j = 0; j < M; ++j) {
    const uint32_t* q = h_win + 5ull * j;
    const uint32_t w = h_w[q[0]], h = h_h[q[0]];
    if (!h_out[j] || h_out_pitch[j] < (uint64_t)q[3] * out_channels) return NICE_E_ARG;
    const uint32_t nx = (w + tile_w - 1) / tile_w, ny = (h + tile_h - 1) / tile_h;
    tab[j] = SetWindow{h_out[j], h_out_pitch[j], q[1], q[2], q[3], q[4], w, h, nx, nx * ny,
                       nice::set_window_mode(h_out[j], h_out_pitch[j], q[1]), 0};
  }
  return NICE_OK;
}
}  // namespace

int nice_set_split_dev(nice_ctx* ctx, void* stream, const uint8_t* const* h_img, const uint64_t* h_pitch,
                       const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint8_t channels, uint32_t tile_w,
                       uint32_t tile_h, uint8_t* d_tiles, uint64_t tile_stride) {
  if (!ctx || !d_tiles || (channels != 3 && channels != 4)) return NICE_E_ARG;
  std::vector<uint32_t> first((size_t)K + 1);
  int rc = nice_set_grid(h_w, h_h, K, tile_w, tile_h, first.data());
  if (rc) return rc;
  if (tile_stride < (uint64_t)tile_w * tile_h * channels) return NICE_E_ARG;
  std::vector<SetImage> tab;
  if ((rc = set_image_table(h_img, h_pitch, h_w, h_h, K, channels, tile_w, first.data(), tab))) return rc;
  NICE_HIP(hipSetDevice(ctx->device));
  if ((rc = ctx->tile_tab.grow(K * sizeof(SetImage)))) return rc;
  NICE_HIP(hipMemcpyAsync(ctx->tile_tab.ptr, tab.data(), K * sizeof(SetImage), hipMemcpyHostToDevice,
                          (hipStream_t)stream));
  return nice::set_split_launch(stream, (const SetImage*)ctx->tile_tab.ptr, K, first[K], channels, tile_w, tile_h,
                                d_tiles, tile_stride);
}

extern "C++" {
namespace {
// What nice_set_merge_dev and nice_set_merge_tensor_dev share, the merge kernel
// alone (ctx, the channels and the call's own arguments checked by the caller);
// Win is the window descriptor of the kernel: the set and the windows
// (table(tab)), the slots, the upload, then launch(d_wins).
template <class Win, class Table, class Launch>
int set_merge_alone(nice_ctx* ctx, void* stream, const uint8_t* d_tiles, uint64_t tile_stride, const uint64_t* d_src_off,
                    const uint32_t* d_slot_win, const uint32_t* d_slot_tile, uint32_t n_slots, uint8_t tile_channels,
                    const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                    const uint32_t* h_win, uint32_t M, Table table, Launch launch) {
  std::vector<uint32_t> slot_first((size_t)M + 1);
  int rc = nice_set_select(h_w, h_h, K, tile_w, tile_h, h_win, M, slot_first.data());
  if (rc) return rc;
  std::vector<Win> tab;
  if ((rc = table(tab))) return rc;
  if (n_slots == 0) return NICE_OK;
  if (!d_tiles || !d_slot_win || !d_slot_tile) return NICE_E_ARG;
  if (!d_src_off && tile_stride < (uint64_t)tile_w * tile_h * tile_channels) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  if ((rc = ctx->tile_tab.grow(M * sizeof(Win)))) return rc;
  NICE_HIP(hipMemcpyAsync(ctx->tile_tab.ptr, tab.data(), M * sizeof(Win), hipMemcpyHostToDevice, (hipStream_t)stream));
  return launch((const Win*)ctx->tile_tab.ptr);
}

// The slots of one merge launch, as set_merge_launch and set_merge_tensor_launch take them.
struct MergeSlots {
  const uint8_t* tiles;
  uint64_t stride;
  const uint64_t* src_off;
  const uint32_t *win, *idx;
  const int32_t* status;
  uint32_t n;
  uint8_t channels;
};
// The tail of nice_decode_set_dev and nice_decode_set_tensor_dev: merge(slots)
// once for the coded slots (decoded, dec_channels bytes per pixel, with their
// statuses) and once for the raw ones (at their offsets in the packed buffer, 3
// bytes per pixel); a kind without slots is not launched.
template <class Merge>
int set_merge_both(const DevSlots& d, const uint8_t* d_packed, uint8_t dec_channels, Merge merge) {
  const MergeSlots both[2] = {{d.dec, d.stride, nullptr, d.c_win, d.c_idx, d.c_st, d.nc, dec_channels},
                              {d_packed, 0, d.s_src, d.s_win, d.s_idx, nullptr, d.ns, 3}};
  for (const MergeSlots& g : both) {
    if (!g.n) continue;
    if (int rc = merge(g)) return rc;
  }
  return NICE_OK;
}
}  // namespace
}  // extern "C++"

int nice_set_merge_dev(nice_ctx* ctx, void* stream, const uint8_t* d_tiles, uint64_t tile_stride,
                       const uint64_t* d_src_off, const uint32_t* d_slot_win, const uint32_t* d_slot_tile,
                       const int32_t* d_slot_status, uint32_t n_slots, uint8_t tile_channels, const uint32_t* h_w,
                       const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h, const uint32_t* h_win,
                       uint8_t* const* h_out, const uint64_t* h_out_pitch, uint32_t M, uint8_t out_channels,
                       uint8_t alpha) {
  if (!ctx) return NICE_E_ARG;
  if ((tile_channels != 3 && tile_channels != 4) || (out_channels != 3 && out_channels != 4)) return NICE_E_ARG;
  if (d_src_off && tile_channels != 3) return NICE_E_ARG;   // (raw tiles in a packed buffer hold 3 bytes per pixel)
  return set_merge_alone<SetWindow>(
      ctx, stream, d_tiles, tile_stride, d_src_off, d_slot_win, d_slot_tile, n_slots, tile_channels, h_w, h_h, K, tile_w,
      tile_h, h_win, M,
      [&](std::vector<SetWindow>& tab) {
        return set_window_table(h_w, h_h, K, tile_w, tile_h, h_win, h_out, h_out_pitch, M, out_channels, tab);
      },
      [&](const SetWindow* d_wins) {
        return nice::set_merge_launch(stream, d_tiles, tile_stride, d_src_off, d_slot_win, d_slot_tile, d_slot_status,
                                      n_slots, d_wins, M, tile_w, tile_h, tile_channels, out_channels, alpha);
      });
}

int nice_encode_set_dev(nice_ctx* ctx, void* stream, const uint8_t* const* h_img, const uint64_t* h_pitch,
                        const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint8_t channels, uint8_t channels_out,
                        uint32_t tile_w, uint32_t tile_h, uint8_t* d_packed, uint64_t packed_cap, uint64_t* d_off,
                        uint64_t* d_len, uint8_t* d_kind, int32_t* d_status) {
  if (!ctx || !d_off || !d_len || !d_kind || !d_status) return NICE_E_ARG;
  if (channels != 3 && channels != 4) return NICE_E_ARG;
  if ((!d_packed && packed_cap) || ((uintptr_t)d_packed & 15)) return NICE_E_ARG;
  std::vector<uint32_t> first((size_t)K + 1);
  int rc = nice_set_grid(h_w, h_h, K, tile_w, tile_h, first.data());
  if (rc) return rc;
  std::vector<SetImage> tab;
  if ((rc = set_image_table(h_img, h_pitch, h_w, h_h, K, channels, tile_w, first.data(), tab))) return rc;
  NICE_HIP(hipSetDevice(ctx->device));
  const uint32_t n = first[K];
  // the small tables: the verify decode's statuses, then the image descriptors
  const size_t o_img = align_up((size_t)n * 4, 16);
  TileEncScratch s;
  if ((rc = tile_enc_scratch(ctx, n, tile_w, tile_h, channels, o_img + K * sizeof(SetImage), s))) return rc;
  const SetImage* d_imgs = (const SetImage*)((uint8_t*)ctx->tile_tab.ptr + o_img);
  NICE_HIP(hipMemcpyAsync((void*)d_imgs, tab.data(), K * sizeof(SetImage), hipMemcpyHostToDevice, (hipStream_t)stream));
  if ((rc = nice::set_split_launch(stream, d_imgs, K, n, channels, tile_w, tile_h, (uint8_t*)ctx->tiles.ptr,
                                   s.tile_stride)))
    return rc;
  return encode_tiles_verified(ctx, stream, n, tile_w, tile_h, channels, channels_out, s, d_packed, packed_cap, d_off,
                               d_len, d_kind, d_status);
}

namespace {
// What nice_decode_set_dev and nice_decode_set_tensor_dev share, up to their
// merges (checked: set and windows, by the caller): the colour plan of the M
// windows, its table behind the window descriptors (`wins`, wins_bytes, a
// multiple of 8), and decode_planned_slots at dec_channels bytes per pixel.
int set_decode_colour(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes, const uint64_t* h_off,
                      const uint64_t* h_len, const uint8_t* h_kind, uint32_t tile_w, uint32_t tile_h,
                      const uint32_t* first, const uint32_t* nx, const uint32_t* h_win, uint32_t M, const void* wins,
                      size_t wins_bytes, uint8_t dec_channels, uint32_t flags, int32_t* d_status, DevSlots& d) {
  plan_colour_slots(SlotTables{h_off, h_len, h_kind, nullptr, packed_bytes},
                    SlotWindows{tile_w, tile_h, first, nx, h_win, M, true}, d.plan);
  ctx->last_set_coded = d.plan.by_kind[0];
  ctx->last_set_raw = d.plan.by_kind[1];
  return decode_planned_slots(ctx, stream, d_packed, packed_bytes, wins, wins_bytes, tile_w, tile_h, dec_channels,
                              (flags & NICE_DEC_ALPHA_FILL_FF) | NICE_DEC_TOLERANT_HEADER, d_status, d);
}
}  // namespace

int nice_decode_set_dev(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                        const uint64_t* h_off, const uint64_t* h_len, const uint8_t* h_kind, const uint32_t* h_w,
                        const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h, const uint32_t* h_win,
                        uint8_t* const* h_out, const uint64_t* h_out_pitch, uint32_t M, uint8_t out_channels,
                        uint32_t flags, int32_t* d_status) {
  if (!ctx || !d_packed || !h_off || !h_len || !h_kind || !d_status) return NICE_E_ARG;
  if (out_channels != 3 && out_channels != 4) return NICE_E_ARG;
  if ((flags & NICE_DEC_STRICT_REFERENCE) || ((uintptr_t)d_packed & 15)) return NICE_E_ARG;
  std::vector<uint32_t> first, nx, slot_first((size_t)M + 1);
  int rc = nice::set_select(h_w, h_h, K, tile_w, tile_h, h_win, M, first, nx, slot_first.data());
  if (rc) return rc;
  std::vector<SetWindow> wins;
  if ((rc = set_window_table(h_w, h_h, K, tile_w, tile_h, h_win, h_out, h_out_pitch, M, out_channels, wins))) return rc;
  NICE_HIP(hipSetDevice(ctx->device));
  DevSlots d;
  if ((rc = set_decode_colour(ctx, stream, d_packed, packed_bytes, h_off, h_len, h_kind, tile_w, tile_h, first.data(),
                              nx.data(), h_win, M, wins.data(), M * sizeof(SetWindow), out_channels, flags, d_status, d)))
    return rc;
  const uint32_t fill = (flags & NICE_DEC_ALPHA_FILL_FF) ? 255u : 0u;   // byte +3 of a raw slot's pixels
  return set_merge_both(d, d_packed, out_channels, [&](const MergeSlots& g) {
    return nice::set_merge_launch(stream, g.tiles, g.stride, g.src_off, g.win, g.idx, g.status, g.n,
                                  (const SetWindow*)d.head, M, tile_w, tile_h, g.channels, out_channels,
                                  g.src_off ? fill : 0u);
  });
}

namespace {
// The output of tensor window j, `width` elements per row and channel
// (h_plane_pitch non-null where planar: the caller's check): NICE_E_ARG for a
// null base, one not aligned to the element, or a row pitch below the row;
// plane_pitch: the window's, 0 where interleaved.
int tensor_out_check(const void* out, uint64_t row_pitch, const uint64_t* h_plane_pitch, uint32_t j, uint32_t width,
                     uint32_t dtype, uint32_t layout, uint64_t& plane_pitch) {
  const bool planar = layout == NICE_TENSOR_PLANAR;
  if (!out || ((uintptr_t)out & (nice::set_tensor_elem_bytes(dtype) - 1))) return NICE_E_ARG;
  if (row_pitch < (uint64_t)width * (planar ? 1u : 3u)) return NICE_E_ARG;
  plane_pitch = planar ? h_plane_pitch[j] : 0;
  return NICE_OK;
}

// The tensor windows of M windows (checked as set_window_table checks its own, and by tensor_out_check).
int set_tensor_window_table(const uint32_t* h_w, const uint32_t* h_h, uint32_t tile_w, uint32_t tile_h,
                            const uint32_t* h_win, const uint8_t* h_flip, void* const* h_out,
                            const uint64_t* h_row_pitch, const uint64_t* h_plane_pitch, uint32_t M, uint32_t dtype,
                            uint32_t layout, std::vector<SetTensorWindow>& tab) {
  if (!h_out || !h_row_pitch || (layout == NICE_TENSOR_PLANAR && !h_plane_pitch)) return NICE_E_ARG;
  tab.resize(M);
  for (uint32_t j = 0; j < M; ++j) {
    const uint32_t* q = h_win + 5ull * j;
    const uint32_t w = h_w[q[0]], h = h_h[q[0]];
    uint64_t pp;
    if (int rc = tensor_out_check(h_out[j], h_row_pitch[j], h_plane_pitch, j, q[3], dtype, layout, pp)) return rc;
    const uint32_t nx = (w + tile_w - 1) / tile_w, ny = (h + tile_h - 1) / tile_h;
    const bool flip = h_flip && h_flip[j];
    tab[j] = SetTensorWindow{h_out[j], h_row_pitch[j], pp, q[1], q[2], q[3], q[4], w, h, nx, nx * ny,
                             nice::set_tensor_window_mode(h_out[j], h_row_pitch[j], pp, q[1], q[3], flip, dtype),
                             flip ? 1u : 0u};
  }
  return NICE_OK;
}

// dtype, layout and the affine constants of a tensor call
int set_tensor_check(uint32_t dtype, uint32_t layout, const float* scale, const float* bias) {
  if (!nice::set_tensor_elem_bytes(dtype)) return NICE_E_ARG;
  if (layout != NICE_TENSOR_PLANAR && layout != NICE_TENSOR_INTERLEAVED) return NICE_E_ARG;
  if (!scale || !bias) return NICE_E_ARG;
  for (int c = 0; c < 3; ++c)
    if (!std::isfinite(scale[c]) || !std::isfinite(bias[c])) return NICE_E_ARG;
  return NICE_OK;
}
}  // namespace

int nice_set_merge_tensor_dev(nice_ctx* ctx, void* stream, const uint8_t* d_tiles, uint64_t tile_stride,
                              const uint64_t* d_src_off, const uint32_t* d_slot_win, const uint32_t* d_slot_tile,
                              const int32_t* d_slot_status, uint32_t n_slots, uint8_t tile_channels, const uint32_t* h_w,
                              const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h, const uint32_t* h_win,
                              const uint8_t* h_flip, void* const* h_out, const uint64_t* h_row_pitch,
                              const uint64_t* h_plane_pitch, uint32_t M, uint32_t dtype, uint32_t layout,
                              const float* scale, const float* bias) {
  if (!ctx) return NICE_E_ARG;
  if (tile_channels != 3 && tile_channels != 4) return NICE_E_ARG;
  if (d_src_off && tile_channels != 3) return NICE_E_ARG;   // (raw tiles in a packed buffer hold 3 bytes per pixel)
  if (int rc = set_tensor_check(dtype, layout, scale, bias)) return rc;
  return set_merge_alone<SetTensorWindow>(
      ctx, stream, d_tiles, tile_stride, d_src_off, d_slot_win, d_slot_tile, n_slots, tile_channels, h_w, h_h, K, tile_w,
      tile_h, h_win, M,
      [&](std::vector<SetTensorWindow>& tab) {
        return set_tensor_window_table(h_w, h_h, tile_w, tile_h, h_win, h_flip, h_out, h_row_pitch, h_plane_pitch, M,
                                       dtype, layout, tab);
      },
      [&](const SetTensorWindow* d_wins) {
        return nice::set_merge_tensor_launch(stream, d_tiles, tile_stride, d_src_off, d_slot_win, d_slot_tile,
                                             d_slot_status, n_slots, d_wins, M, tile_w, tile_h, tile_channels, dtype,
                                             layout, scale, bias);
      });
}

int nice_decode_set_tensor_dev(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                               const uint64_t* h_off, const uint64_t* h_len, const uint8_t* h_kind,
                               const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                               const uint32_t* h_win, const uint8_t* h_flip, void* const* h_out,
                               const uint64_t* h_row_pitch, const uint64_t* h_plane_pitch, uint32_t M, uint32_t dtype,
                               uint32_t layout, const float* scale, const float* bias, uint32_t flags,
                               int32_t* d_status) {
  if (!ctx || !d_packed || !h_off || !h_len || !h_kind || !d_status) return NICE_E_ARG;
  if ((flags & NICE_DEC_STRICT_REFERENCE) || ((uintptr_t)d_packed & 15)) return NICE_E_ARG;
  int rc = set_tensor_check(dtype, layout, scale, bias);
  if (rc) return rc;
  std::vector<uint32_t> first, nx, slot_first((size_t)M + 1);
  if ((rc = nice::set_select(h_w, h_h, K, tile_w, tile_h, h_win, M, first, nx, slot_first.data()))) return rc;
  std::vector<SetTensorWindow> wins;
  if ((rc = set_tensor_window_table(h_w, h_h, tile_w, tile_h, h_win, h_flip, h_out, h_row_pitch, h_plane_pitch, M, dtype,
                                    layout, wins)))
    return rc;
  NICE_HIP(hipSetDevice(ctx->device));
  // the coded slots at 4 bytes per pixel, whatever the set's channels: a lane loads dwords
  DevSlots d;
  if ((rc = set_decode_colour(ctx, stream, d_packed, packed_bytes, h_off, h_len, h_kind, tile_w, tile_h, first.data(),
                              nx.data(), h_win, M, wins.data(), M * sizeof(SetTensorWindow), 4, flags, d_status, d)))
    return rc;
  ctx->last_set_merges = (d.nc ? 1u : 0u) + (d.ns ? 1u : 0u);
  return set_merge_both(d, d_packed, 4, [&](const MergeSlots& g) {
    return nice::set_merge_tensor_launch(stream, g.tiles, g.stride, g.src_off, g.win, g.idx, g.status, g.n,
                                         (const SetTensorWindow*)d.head, M, tile_w, tile_h, g.channels, dtype, layout,
                                         scale, bias);
  });
}

// ---- image sets: resized tensor output ------------------------------------------
namespace {
// The resize windows of M windows (set and windows checked: set_select, which
// gave slot_first): outputs of out_h x out_w per channel, checked as
// set_tensor_window_table checks its own.
int set_resize_window_table(const uint32_t* h_w, const uint32_t* h_h, uint32_t tile_w, uint32_t tile_h,
                            const uint32_t* h_win, const uint8_t* h_flip, const uint32_t* slot_first, uint32_t out_w,
                            uint32_t out_h, void* const* h_out, const uint64_t* h_row_pitch,
                            const uint64_t* h_plane_pitch, uint32_t M, uint32_t dtype, uint32_t layout,
                            std::vector<SetResizeWindow>& tab) {
  if (out_w == 0 || out_h == 0 || out_w > nice::RESIZE_MAX_OUT || out_h > nice::RESIZE_MAX_OUT) return NICE_E_ARG;
  if (!h_out || !h_row_pitch || (layout == NICE_TENSOR_PLANAR && !h_plane_pitch)) return NICE_E_ARG;
  tab.resize(M);
  for (uint32_t j = 0; j < M; ++j) {
    const uint32_t* q = h_win + 5ull * j;
    uint64_t pp;
    if (int rc = tensor_out_check(h_out[j], h_row_pitch[j], h_plane_pitch, j, out_w, dtype, layout, pp)) return rc;
    const TileRange r = nice::window_tiles(tile_w, tile_h, q[1], q[2], q[3], q[4]);
    tab[j] = SetResizeWindow{h_out[j], h_row_pitch[j], pp, q[1], q[2], q[3], q[4], r.tx0, r.ty0, r.tx1 - r.tx0,
                             slot_first[j], nice::set_resize_window_mode(h_out[j], h_row_pitch[j], pp, dtype),
                             (h_flip && h_flip[j]) ? 1u : 0u};
  }
  return NICE_OK;
}
}  // namespace

extern "C++" {
namespace {
// What the resize entry points share; Win is the window descriptor of the kernel.
// The kernel alone: the checks, the windows (table(slot_first, tab)), their
// upload, then launch(d_wins).
template <class Win, class Table, class Launch>
int set_resize_alone(nice_ctx* ctx, void* stream, const uint8_t* d_tiles, uint64_t tile_stride, const uint64_t* d_src,
                     const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                     const uint32_t* h_win, uint32_t M, uint32_t dtype, uint32_t layout, const float* scale,
                     const float* bias, Table table, Launch launch) {
  if (!ctx || !d_src) return NICE_E_ARG;
  int rc = set_tensor_check(dtype, layout, scale, bias);
  if (rc) return rc;
  std::vector<uint32_t> slot_first((size_t)M + 1);
  if ((rc = nice_set_select(h_w, h_h, K, tile_w, tile_h, h_win, M, slot_first.data()))) return rc;
  std::vector<Win> tab;
  if ((rc = table(slot_first.data(), tab))) return rc;
  // dense slots are read as dwords
  if (d_tiles && (!nice::tl_aligned(d_tiles, tile_stride, 4) || tile_stride < (uint64_t)tile_w * tile_h * 4))
    return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  if ((rc = ctx->tile_tab.grow(M * sizeof(Win)))) return rc;
  NICE_HIP(hipMemcpyAsync(ctx->tile_tab.ptr, tab.data(), M * sizeof(Win), hipMemcpyHostToDevice, (hipStream_t)stream));
  return launch((const Win*)ctx->tile_tab.ptr);
}

// The whole call: the checks, the windows, the plan with its position column
// behind the window descriptors in the head, one upload, one batch decode of
// the coded slots at 4 bytes per pixel (a tap or a staged pixel is one dword),
// one status scatter, then launch(d, d_wins, d_src), which makes `launches` launches.
template <class Win, class Table, class Launch>
int set_decode_resized(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes, const uint64_t* h_off,
                       const uint64_t* h_len, const uint8_t* h_kind, const uint32_t* h_w, const uint32_t* h_h, uint32_t K,
                       uint32_t tile_w, uint32_t tile_h, const uint32_t* h_win, uint32_t M, uint32_t dtype,
                       uint32_t layout, const float* scale, const float* bias, uint32_t flags, int32_t* d_status,
                       uint32_t launches, Table table, Launch launch) {
  if (!ctx || !d_packed || !h_off || !h_len || !h_kind || !d_status) return NICE_E_ARG;
  if ((flags & NICE_DEC_STRICT_REFERENCE) || ((uintptr_t)d_packed & 15)) return NICE_E_ARG;
  int rc = set_tensor_check(dtype, layout, scale, bias);
  if (rc) return rc;
  std::vector<uint32_t> first, nx, slot_first((size_t)M + 1);
  if ((rc = nice::set_select(h_w, h_h, K, tile_w, tile_h, h_win, M, first, nx, slot_first.data()))) return rc;
  std::vector<Win> wins;
  if ((rc = table(slot_first.data(), wins))) return rc;
  NICE_HIP(hipSetDevice(ctx->device));
  // the plan first: its position column travels in the head, behind the window descriptors
  DevSlots d;
  plan_colour_slots(SlotTables{h_off, h_len, h_kind, nullptr, packed_bytes},
                    SlotWindows{tile_w, tile_h, first.data(), nx.data(), h_win, M, true}, d.plan);
  ctx->last_set_coded = d.plan.by_kind[0];
  ctx->last_set_raw = d.plan.by_kind[1];
  std::vector<uint64_t> src;
  nice::slot_position_sources(d.plan, src);
  const size_t wins_bytes = M * sizeof(Win);
  std::vector<uint8_t> head(wins_bytes + 8 * src.size());
  memcpy(head.data(), wins.data(), wins_bytes);
  if (!src.empty()) memcpy(head.data() + wins_bytes, src.data(), 8 * src.size());
  if ((rc = decode_planned_slots(ctx, stream, d_packed, packed_bytes, head.data(), head.size(), tile_w, tile_h, 4,
                                 (flags & NICE_DEC_ALPHA_FILL_FF) | NICE_DEC_TOLERANT_HEADER, d_status, d)))
    return rc;
  ctx->last_set_merges = launches;
  return launch(d, (const Win*)d.head, (const uint64_t*)(d.head + wins_bytes));
}
}  // namespace
}  // extern "C++"

int nice_set_resize_tensor_dev(nice_ctx* ctx, void* stream, const uint8_t* d_tiles, uint64_t tile_stride,
                               const uint8_t* d_packed, const uint64_t* d_src, const int32_t* d_slot_status,
                               const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                               const uint32_t* h_win, const uint8_t* h_flip, uint32_t out_w, uint32_t out_h,
                               void* const* h_out, const uint64_t* h_row_pitch, const uint64_t* h_plane_pitch,
                               uint32_t M, uint32_t dtype, uint32_t layout, const float* scale, const float* bias) {
  return set_resize_alone<SetResizeWindow>(
      ctx, stream, d_tiles, tile_stride, d_src, h_w, h_h, K, tile_w, tile_h, h_win, M, dtype, layout, scale, bias,
      [&](const uint32_t* slot_first, std::vector<SetResizeWindow>& tab) {
        return set_resize_window_table(h_w, h_h, tile_w, tile_h, h_win, h_flip, slot_first, out_w, out_h, h_out,
                                       h_row_pitch, h_plane_pitch, M, dtype, layout, tab);
      },
      [&](const SetResizeWindow* d_wins) {
        return nice::set_resize_tensor_launch(stream, d_tiles, tile_stride, d_packed, d_src, d_slot_status, d_wins, M,
                                              tile_w, tile_h, out_w, out_h, dtype, layout, scale, bias);
      });
}

int nice_decode_set_resized_dev(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                                const uint64_t* h_off, const uint64_t* h_len, const uint8_t* h_kind,
                                const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                                const uint32_t* h_win, const uint8_t* h_flip, uint32_t out_w, uint32_t out_h,
                                void* const* h_out, const uint64_t* h_row_pitch, const uint64_t* h_plane_pitch,
                                uint32_t M, uint32_t dtype, uint32_t layout, const float* scale, const float* bias,
                                uint32_t flags, int32_t* d_status) {
  return set_decode_resized<SetResizeWindow>(
      ctx, stream, d_packed, packed_bytes, h_off, h_len, h_kind, h_w, h_h, K, tile_w, tile_h, h_win, M, dtype, layout,
      scale, bias, flags, d_status, 1,
      [&](const uint32_t* slot_first, std::vector<SetResizeWindow>& tab) {
        return set_resize_window_table(h_w, h_h, tile_w, tile_h, h_win, h_flip, slot_first, out_w, out_h, h_out,
                                       h_row_pitch, h_plane_pitch, M, dtype, layout, tab);
      },
      [&](const DevSlots& d, const SetResizeWindow* d_wins, const uint64_t* d_src) {
        return nice::set_resize_tensor_launch(stream, d.dec, d.stride, d_packed, d_src, d_status, d_wins, M, tile_w,
                                              tile_h, out_w, out_h, dtype, layout, scale, bias);
      });
}

// ---- image sets: antialiased resized tensor output -------------------------------
namespace {
// The windows of the antialiased resize (checked as set_resize_window_table
// checks its own; NICE_E_ARG also for a reducing axis above
// NICE_RESIZE_AA_MAX_IN), the entries of their weight tables and the longest
// reducing axis.
int set_resize_aa_window_table(const uint32_t* h_w, const uint32_t* h_h, uint32_t tile_w, uint32_t tile_h,
                               const uint32_t* h_win, const uint8_t* h_flip, const uint32_t* slot_first,
                               uint32_t out_w, uint32_t out_h, void* const* h_out, const uint64_t* h_row_pitch,
                               const uint64_t* h_plane_pitch, uint32_t M, uint32_t dtype, uint32_t layout,
                               std::vector<SetResizeAaWindow>& tab, uint64_t& entries, uint32_t& max_reducing) {
  std::vector<SetResizeWindow> plain;
  int rc = set_resize_window_table(h_w, h_h, tile_w, tile_h, h_win, h_flip, slot_first, out_w, out_h, h_out, h_row_pitch,
                                   h_plane_pitch, M, dtype, layout, plain);
  if (rc) return rc;
  tab.resize(M);
  entries = 0;
  max_reducing = 0;
  for (uint32_t j = 0; j < M; ++j) {
    const SetResizeWindow& p = plain[j];
    if (!nice::resize_aa_axis_ok(p.rw, out_w) || !nice::resize_aa_axis_ok(p.rh, out_h)) return NICE_E_ARG;
    const uint64_t nc = nice::set_resize_aa_table_entries(p.rw, out_w), nr = nice::set_resize_aa_table_entries(p.rh, out_h);
    if (entries + nc + nr > 0xFFFFFFFFull) return NICE_E_ARG;
    tab[j] = SetResizeAaWindow{p.out, p.row_pitch, p.plane_pitch, p.x0, p.y0, p.rw, p.rh, p.tx0, p.ty0, p.ntx,
                               p.slot_first, (uint32_t)entries, (uint32_t)(entries + nc), p.flip, 0u};
    entries += nc + nr;
    if (nc) max_reducing = std::max(max_reducing, p.rw);
    if (nr) max_reducing = std::max(max_reducing, p.rh);
  }
  return NICE_OK;
}
}  // namespace

int nice_set_resize_aa_tensor_dev(nice_ctx* ctx, void* stream, const uint8_t* d_tiles, uint64_t tile_stride,
                                  const uint8_t* d_packed, const uint64_t* d_src, const int32_t* d_slot_status,
                                  const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w,
                                  uint32_t tile_h, const uint32_t* h_win, const uint8_t* h_flip, uint32_t out_w,
                                  uint32_t out_h, void* const* h_out, const uint64_t* h_row_pitch,
                                  const uint64_t* h_plane_pitch, uint32_t M, uint32_t dtype, uint32_t layout,
                                  const float* scale, const float* bias) {
  uint64_t entries = 0;
  uint32_t max_reducing = 0;
  return set_resize_alone<SetResizeAaWindow>(
      ctx, stream, d_tiles, tile_stride, d_src, h_w, h_h, K, tile_w, tile_h, h_win, M, dtype, layout, scale, bias,
      [&](const uint32_t* slot_first, std::vector<SetResizeAaWindow>& tab) {
        return set_resize_aa_window_table(h_w, h_h, tile_w, tile_h, h_win, h_flip, slot_first, out_w, out_h, h_out,
                                          h_row_pitch, h_plane_pitch, M, dtype, layout, tab, entries, max_reducing);
      },
      [&](const SetResizeAaWindow* d_wins) {
        if (int rc = ctx->aa_weights.grow(std::max<size_t>(2 * entries, 16))) return rc;
        return nice::set_resize_aa_tensor_launch(stream, d_tiles, tile_stride, d_packed, d_src, d_slot_status, d_wins, M,
                                                 (uint16_t*)ctx->aa_weights.ptr, max_reducing, tile_w, tile_h, out_w,
                                                 out_h, dtype, layout, scale, bias);
      });
}

int nice_decode_set_resized_aa_dev(nice_ctx* ctx, void* stream, const uint8_t* d_packed, uint64_t packed_bytes,
                                   const uint64_t* h_off, const uint64_t* h_len, const uint8_t* h_kind,
                                   const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w,
                                   uint32_t tile_h, const uint32_t* h_win, const uint8_t* h_flip, uint32_t out_w,
                                   uint32_t out_h, void* const* h_out, const uint64_t* h_row_pitch,
                                   const uint64_t* h_plane_pitch, uint32_t M, uint32_t dtype, uint32_t layout,
                                   const float* scale, const float* bias, uint32_t flags, int32_t* d_status) {
  uint64_t entries = 0;
  uint32_t max_reducing = 0;
  return set_decode_resized<SetResizeAaWindow>(
      ctx, stream, d_packed, packed_bytes, h_off, h_len, h_kind, h_w, h_h, K, tile_w, tile_h, h_win, M, dtype, layout,
      scale, bias, flags, d_status, 2,   // the weight tables, the filter
      [&](const uint32_t* slot_first, std::vector<SetResizeAaWindow>& tab) {
        return set_resize_aa_window_table(h_w, h_h, tile_w, tile_h, h_win, h_flip, slot_first, out_w, out_h, h_out,
                                          h_row_pitch, h_plane_pitch, M, dtype, layout, tab, entries, max_reducing);
      },
      [&](const DevSlots& d, const SetResizeAaWindow* d_wins, const uint64_t* d_src) {
        if (int rc = ctx->aa_weights.grow(std::max<size_t>(2 * entries, 16))) return rc;
        return nice::set_resize_aa_tensor_launch(stream, d.dec, d.stride, d_packed, d_src, d_status, d_wins, M,
                                                 (uint16_t*)ctx->aa_weights.ptr, max_reducing, tile_w, tile_h, out_w,
                                                 out_h, dtype, layout, scale, bias);
      });
}

// ---- image sets: the alpha batch ---------------------------------------------
uint64_t nice_set_alpha_bound(const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h) {
  std::vector<uint32_t> first((size_t)K + 1);
  if (nice_set_grid(h_w, h_h, K, tile_w, tile_h, first.data())) return 0;
  const uint64_t per = std::max<uint64_t>(nice_encode_bound(nice_tile_alpha_width(tile_w), tile_h),
                                          (uint64_t)tile_w * tile_h);
  return (uint64_t)first[K] * align_up(per, 16);
}

int nice_set_alpha_range_dev(nice_ctx* ctx, void* stream, const uint8_t* const* h_img, const uint64_t* h_pitch,
                             const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                             uint32_t* d_lo, uint32_t* d_hi) {
  if (!ctx || !d_lo || !d_hi) return NICE_E_ARG;
  std::vector<uint32_t> first((size_t)K + 1);
  int rc = nice_set_grid(h_w, h_h, K, tile_w, tile_h, first.data());
  if (rc) return rc;
  std::vector<SetImage> tab;
  if ((rc = set_image_table(h_img, h_pitch, h_w, h_h, K, 4, tile_w, first.data(), tab))) return rc;
  NICE_HIP(hipSetDevice(ctx->device));
  if ((rc = ctx->tile_tab.grow(K * sizeof(SetImage)))) return rc;
  NICE_HIP(hipMemcpyAsync(ctx->tile_tab.ptr, tab.data(), K * sizeof(SetImage), hipMemcpyHostToDevice,
                          (hipStream_t)stream));
  return nice::set_alpha_range_launch(stream, (const SetImage*)ctx->tile_tab.ptr, K, first[K], tile_w, tile_h, d_lo,
                                      d_hi);
}

int nice_encode_set_alpha_dev(nice_ctx* ctx, void* stream, const uint8_t* const* h_img, const uint64_t* h_pitch,
                              const uint32_t* h_w, const uint32_t* h_h, uint32_t K, uint32_t tile_w, uint32_t tile_h,
                              uint8_t* d_apacked, uint64_t apacked_cap, uint64_t* d_aoff, uint64_t* d_alen,
                              uint8_t* d_akind, uint8_t* d_aval, int32_t* d_status) {
  if (!ctx || !d_aoff || !d_alen || !d_akind || !d_aval || !d_status) return NICE_E_ARG;
  if ((!d_apacked && apacked_cap) || ((uintptr_t)d_apacked & 15)) return NICE_E_ARG;
  std::vector<uint32_t> first((size_t)K + 1);
  int rc = nice_set_grid(h_w, h_h, K, tile_w, tile_h, first.data());
  if (rc) return rc;
  std::vector<SetImage> imgs;
  if ((rc = set_image_table(h_img, h_pitch, h_w, h_h, K, 4, tile_w, first.data(), imgs))) return rc;
  NICE_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  // the small tables of the alpha encode, then the image descriptors
  AlphaEnc a(first[K]);
  if ((rc = ctx->tile_tab.grow(a.end + K * sizeof(SetImage)))) return rc;
  uint8_t* dt = (uint8_t*)ctx->tile_tab.ptr;
  const SetImage* d_imgs = (const SetImage*)(dt + a.end);
  NICE_HIP(hipMemcpyAsync((void*)d_imgs, imgs.data(), K * sizeof(SetImage), hipMemcpyHostToDevice, st));
  if ((rc = nice::set_alpha_range_launch(stream, d_imgs, K, a.n, tile_w, tile_h, (uint32_t*)(dt + a.o_lo),
                                         (uint32_t*)(dt + a.o_hi))))
    return rc;
  if ((rc = alpha_encode_classify(ctx, st, tile_w, tile_h, a, d_alen, d_akind, d_aval))) return rc;
  if (a.m && (rc = nice::set_alpha_gather_launch(stream, d_imgs, K, tile_w, tile_h, (const uint32_t*)(dt + a.o_list),
                                                 a.m, (uint8_t*)ctx->tiles.ptr, a.trip_stride)))
    return rc;
  return alpha_encode_finish(ctx, stream, tile_w, tile_h, a, d_apacked, apacked_cap, d_aoff, d_alen, d_akind, d_status);
}

int nice_decode_set_alpha_dev(nice_ctx* ctx, void* stream, const uint8_t* d_apacked, uint64_t apacked_bytes,
                              const uint64_t* h_aoff, const uint64_t* h_alen, const uint8_t* h_akind,
                              const uint8_t* h_aval, const uint32_t* h_w, const uint32_t* h_h, uint32_t K,
                              uint32_t tile_w, uint32_t tile_h, const uint32_t* h_win, uint8_t* const* h_out,
                              const uint64_t* h_out_pitch, uint32_t M, int32_t* d_status) {
  if (!ctx || !h_aoff || !h_alen || !h_akind || !h_aval || !d_status) return NICE_E_ARG;
  if ((!d_apacked && apacked_bytes) || ((uintptr_t)d_apacked & 15)) return NICE_E_ARG;
  std::vector<uint32_t> first, nx, slot_first((size_t)M + 1);
  int rc = nice::set_select(h_w, h_h, K, tile_w, tile_h, h_win, M, first, nx, slot_first.data());
  if (rc) return rc;
  std::vector<SetWindow> wins;
  if ((rc = set_window_table(h_w, h_h, K, tile_w, tile_h, h_win, h_out, h_out_pitch, M, 4, wins))) return rc;
  NICE_HIP(hipSetDevice(ctx->device));
  // every (window, tile) pair is a slot: the coded ones to decode, and every
  // accepted slot to merge with its source
  DevSlots d;
  plan_alpha_slots(SlotTables{h_aoff, h_alen, h_akind, h_aval, apacked_bytes},
                   SlotWindows{tile_w, tile_h, first.data(), nx.data(), h_win, M, true}, d.plan);
  ctx->last_set_alpha_coded = d.plan.by_kind[0];
  ctx->last_set_alpha_raw = d.plan.by_kind[1];
  ctx->last_set_alpha_const = d.plan.by_kind[2];
  if ((rc = decode_planned_slots(ctx, stream, d_apacked, apacked_bytes, wins.data(), M * sizeof(SetWindow),
                                 nice_tile_alpha_width(tile_w), tile_h, 3, NICE_DEC_TOLERANT_HEADER, d_status, d)))
    return rc;
  return nice::set_alpha_merge_launch(stream, d.dec, d.stride, d.c_st, d_apacked, d.s_src, d.s_kind, d.s_win, d.s_idx,
                                      d.ns, (const SetWindow*)d.head, M, tile_w, tile_h);
}

// ---- one image sharded over ranks ------------------------
int nice_band_classify(nice_ctx* ctx, void* stream, const uint8_t* d_px, uint64_t px0, uint64_t px_count,
                       uint32_t w, uint32_t h, uint8_t channels, uint8_t channels_out, uint32_t tile_lo,
                       uint32_t tile_hi, uint32_t* d_edges) {
  if (!ctx || !d_px || !d_edges || (channels != 3 && channels != 4)) return NICE_E_ARG;
  const uint64_t N = (uint64_t)w * h;
  const uint32_t T = enc_tiles(w, h);
  if (N == 0 || N > (1ull << 30) || tile_lo >= tile_hi || tile_hi > T) return NICE_E_ARG;
  // pixel memory must hold the band and the 3 rows + 3 pixels its references reach
  const uint64_t band_px0 = (uint64_t)tile_lo * ENC_TILE;
  const uint64_t band_px1 = std::min<uint64_t>((uint64_t)tile_hi * ENC_TILE, N);
  const uint64_t need0 = band_px0 > 3ull * w + 3 ? band_px0 - 3ull * w - 3 : 0;
  if (px0 > need0 || px0 + px_count < band_px1 || px0 + px_count > N) return NICE_E_ARG;
  if (channels == 4 && ((uintptr_t)d_px & 3)) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  EncLayout L = enc_layout(1, T, band_px1 - band_px0);
  int rc = ctx->band.grow(L.total);
  if (rc) return rc;
  uint8_t* base = (uint8_t*)ctx->band.ptr;
  // virtual base: global pixel index g addresses d_px + (g - px0) * channels
  const uint8_t* vpx = d_px - (int64_t)px0 * channels;
  EncShape shape{};
  shape.n_frames = 1;
  shape.w = w;
  shape.h = h;
  shape.channels = channels;
  shape.cus = ctx->cus;
  // the ring / strip kernels read the band's pixels through the virtual base
  // as 32-bit words: it must be 4-byte aligned
  shape.aligned4 = ((uintptr_t)vpx & 3) == 0;
  shape.aligned16 = ((uintptr_t)vpx & 15) == 0;
  shape.band = true;
  shape.tile_lo = tile_lo;
  shape.tile_hi = tile_hi;
  const EncPlan P = plan_encode(shape, enc_opts());
  // one-pass packer with look-back from band_bit0; FLAG_LONG bands take the
  // long-code path (tile bits, their scan) like frames
  EncArgs a = enc_args(ctx, L, base, P, 1, w, h, channels, channels_out);
  a.px = vpx;
  a.frame_stride = 0;
  a.recs = (uint32_t*)(base + L.o_recs) - band_px0;   // band records are stored from the band's first pixel
  a.px_lo = (int64_t)px0;
  a.px_hi = (int64_t)(px0 + px_count);
  a.band = 1;
  NICE_HIP(hipMemsetAsync(base, 0, L.zero_bytes, st));
  if ((rc = launch_classify(P, a, st))) return rc;
  ctx->last_classify = (int)P.kind;
  hipLaunchKernelGGL(enc_band_edges, dim3(1), dim3(BAND_THREADS), 0, st, a, d_edges);
  NICE_HIP(hipGetLastError());
  ctx->bs = BandState{};
  ctx->bs.a = a;
  ctx->bs.plan = P;
  ctx->bs.bhist = (uint32_t*)(base + L.o_bhist);
  ctx->bs.classified = true;
  return NICE_OK;
}

static int band_runs(nice_ctx* ctx, void* stream, uint32_t band_next, const uint32_t* d_band_next,
                     uint32_t* d_hist) {
  if (!ctx || !d_hist || !ctx->bs.classified) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  EncArgs& a = ctx->bs.a;
  a.band_next = band_next;
  a.band_next_dev = d_band_next;
  launch_runs(ctx->bs.plan, a, st);
  a.band_next_dev = nullptr;
  NICE_HIP(hipMemcpyAsync(ctx->bs.bhist, a.hist, N_BINS * 4, hipMemcpyDeviceToDevice, st));
  NICE_HIP(hipMemcpyAsync(d_hist, a.hist, N_BINS * 4, hipMemcpyDeviceToDevice, st));
  NICE_HIP(hipGetLastError());
  return NICE_OK;
}

int nice_band_runs(nice_ctx* ctx, void* stream, uint32_t band_next, uint32_t* d_hist) {
  return band_runs(ctx, stream, band_next, nullptr, d_hist);
}

int nice_band_runs_dev(nice_ctx* ctx, void* stream, const uint32_t* d_band_next, uint32_t* d_hist) {
  if (!d_band_next) return NICE_E_ARG;
  return band_runs(ctx, stream, 0, d_band_next, d_hist);
}

// Code tables from the summed histogram, the header into the context's header
// buffer, the band's bit count and the data start into d_info (device).
static int band_tables(nice_ctx* ctx, hipStream_t st, const uint32_t* d_hist_total, unsigned long long* d_info) {
  EncArgs& a = ctx->bs.a;
  NICE_HIP(hipMemcpyAsync(a.hist, d_hist_total, N_BINS * 4, hipMemcpyDeviceToDevice, st));
  const EncPlan& P = ctx->bs.plan;
  hipLaunchKernelGGL(enc_tables, grid_of(P.tables), dim3(P.tables.threads), 0, st, a);
  EncArgs h = a;   // the header goes to the context's header buffer
  h.out = (uint8_t*)ctx->band_hdr.ptr;
  h.out_stride = 4096;
  h.out_len = (unsigned long long*)((uint8_t*)ctx->band_hdr.ptr + 4096);
  hipLaunchKernelGGL(enc_header, grid_of(P.header), dim3(P.header.threads), 0, st, h);
  hipLaunchKernelGGL(enc_packtab, grid_of(P.packtab), dim3(P.packtab.threads), 0, st, a);
  hipLaunchKernelGGL(enc_band_sum, dim3(1), dim3(BAND_THREADS), 0, st, a, (const uint32_t*)ctx->bs.bhist, d_info);
  NICE_HIP(hipGetLastError());
  return NICE_OK;
}

int nice_band_tables(nice_ctx* ctx, void* stream, const uint32_t* d_hist_total, uint64_t* band_bits,
                     uint64_t* seed_bit) {
  if (!ctx || !d_hist_total || !ctx->bs.classified) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  int rc = ctx->band_hdr.grow(4096 + 64);
  if (rc) return rc;
  unsigned long long* info = (unsigned long long*)((uint8_t*)ctx->band_hdr.ptr + 4096 + 16);
  if ((rc = band_tables(ctx, st, d_hist_total, info))) return rc;
  unsigned long long hinfo[2];
  NICE_HIP(hipMemcpyAsync(hinfo, info, 16, hipMemcpyDeviceToHost, st));
  NICE_HIP(hipStreamSynchronize(st));
  ctx->bs.band_bits = hinfo[0];
  ctx->bs.seed_bit = hinfo[1];
  ctx->bs.tabled = true;
  if (band_bits) *band_bits = hinfo[0];
  if (seed_bit) *seed_bit = hinfo[1];
  return NICE_OK;
}

int nice_band_tables_dev(nice_ctx* ctx, void* stream, const uint32_t* d_hist_total, uint64_t* d_info) {
  if (!ctx || !d_hist_total || !d_info || !ctx->bs.classified) return NICE_E_ARG;
  NICE_HIP(hipSetDevice(ctx->device));
  int rc = ctx->band_hdr.grow(4096 + 64);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = band_tables(ctx, st, d_hist_total, (unsigned long long*)d_info))) return rc;
  // the context's own copy: the caller's buffer may be freed or reused before the pack
  unsigned long long* mine = (unsigned long long*)((uint8_t*)ctx->band_hdr.ptr + 4096 + 32);
  NICE_HIP(hipMemcpyAsync(mine, d_info, 16, hipMemcpyDeviceToDevice, st));
  ctx->bs.tabled = true;
  ctx->bs.band_bits = ~0ull;   // known to the caller once d_info is read (nice_band_pack_bits)
  ctx->bs.seed_bit = ~0ull;
  ctx->bs.d_info = mine;
  return NICE_OK;
}

uint32_t nice_tile_pixels(void) { return ENC_TILE; }

// the stream words the band touches, then a two-word trailer (a deferred
// wrapped write, enc_band_fix)
static uint64_t band_data_words(uint64_t band_bit0, uint64_t band_bits) {
  return band_bits ? ((band_bit0 + band_bits + 31) >> 5) - (band_bit0 >> 5) : 0;
}

uint64_t nice_band_words(uint64_t band_bit0, uint64_t band_bits) {
  return band_data_words(band_bit0, band_bits) + 2;   // every band has its trailer (status, deferred write)
}

int nice_band_pack_bits(nice_ctx* ctx, void* stream, uint64_t band_bit0, uint64_t band_bits, uint32_t* d_words,
                        uint64_t words_cap) {
  if (!ctx || !ctx->bs.tabled) return NICE_E_ARG;
  const uint64_t nw = nice_band_words(band_bit0, band_bits);
  if (nw > words_cap || (nw && !d_words)) return NICE_E_ARG;
  if (ctx->bs.seed_bit != ~0ull && band_bit0 < ctx->bs.seed_bit) return NICE_E_ARG;
  ctx->bs.band_bits = band_bits;
  NICE_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  EncArgs a = ctx->bs.a;
  a.band_bit0 = band_bit0;
  a.out = (uint8_t*)d_words - (int64_t)(band_bit0 >> 5) * 4;   // virtual: stream word w at d_words[w - w0]
  a.out_stride = 0;
  a.band_fix = d_words + (nw - 2);
  NICE_HIP(hipMemsetAsync(a.band_fix, 0, 8, st));
  // the bit count the caller read back must be the device's: on a mismatch the
  // pack kernels skip the band and the trailer carries BAND_FIX_BAD, which
  // nice_band_assemble reports
  if (ctx->bs.d_info)
    hipLaunchKernelGGL(enc_band_check, dim3(1), dim3(ENC_WAVE_THREADS), 0, st, a, ctx->bs.d_info,
                       (unsigned long long)band_bits);
  if (band_bits == 0) {   // no data words: the trailer only
    NICE_HIP(hipGetLastError());
    return NICE_OK;
  }
  // the first word holds the previous band's last bits: only OR-ed into (enc_edges)
  NICE_HIP(hipMemsetAsync(d_words, 0, 4, st));
  const uint32_t nt = a.tile_hi - a.tile_lo;
  const uint32_t ng = (nt + PACK_SUB - 1) / PACK_SUB;
  NICE_HIP(hipMemsetAsync(a.status, 0, (size_t)ng * 8, st));
  NICE_HIP(hipMemsetAsync(a.pack_ctr, 0, 4, st));
  NICE_HIP(hipMemsetAsync(a.over_count, 0, 4, st));
  // the scan and the look-back start from band_bit0
  launch_pack(ctx->bs.plan, a, st, nullptr);
  NICE_HIP(hipGetLastError());
  return NICE_OK;
}

int nice_band_pack(nice_ctx* ctx, void* stream, uint64_t band_bit0, uint32_t* d_words, uint64_t words_cap) {
  if (!ctx || !ctx->bs.tabled || ctx->bs.band_bits == ~0ull) return NICE_E_ARG;
  return nice_band_pack_bits(ctx, stream, band_bit0, ctx->bs.band_bits, d_words, words_cap);
}

int nice_band_assemble(nice_ctx* ctx, void* stream, const uint32_t* d_words, const uint64_t* band_bit0,
                       const uint64_t* band_bits, uint32_t n_bands, uint8_t* d_out, uint64_t out_cap,
                       uint64_t* out_len) {
  if (!ctx || !ctx->bs.tabled || !d_out || !out_len || n_bands == 0 || !band_bit0 || !band_bits)
    return NICE_E_ARG;
  // the data start: learned by nice_band_tables, else the first band's start
  const uint64_t seed = ctx->bs.seed_bit != ~0ull ? ctx->bs.seed_bit : band_bit0[0];
  // meta: band first words [R], band offsets [R + 1], data end, out_len, band first bits [R],
  // status (a band's trailer marked BAND_FIX_BAD: its pack saw a wrong band_bits)
  std::vector<unsigned long long> meta(3 * n_bands + 4);
  uint64_t off = 0, end = seed;
  for (uint32_t r = 0; r < n_bands; ++r) {
    if (band_bit0[r] != end) return NICE_E_ARG;   // bands must tile the data bits
    meta[r] = band_bit0[r] >> 5;
    meta[n_bands + r] = off;
    meta[2 * n_bands + 3 + r] = band_bit0[r];
    off += nice_band_words(band_bit0[r], band_bits[r]);
    end += band_bits[r];
  }
  meta[2 * n_bands] = off;
  meta[2 * n_bands + 1] = end;
  const uint64_t B = end >> 3;
  if (B + 5 > out_cap || (((uintptr_t)d_out) & 3)) return NICE_E_CAPACITY;
  NICE_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  int rc = ctx->dev_len.grow(meta.size() * 8 + 64);
  if (rc) return rc;
  unsigned long long* dmeta = (unsigned long long*)ctx->dev_len.ptr;
  NICE_HIP(hipMemcpyAsync(dmeta, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, st));
  // header words (the last one zero padded), then the bands, then the tail
  NICE_HIP(hipMemcpyAsync(d_out, ctx->band_hdr.ptr, ((seed + 31) >> 5) * 4, hipMemcpyDeviceToDevice, st));
  // words past the header up to the end are written by the bands (first/last OR-ed)
  const uint64_t hdr_words = (seed + 31) >> 5, end_words = (end + 31) >> 5;
  if (end_words > hdr_words)
    NICE_HIP(hipMemsetAsync(d_out + hdr_words * 4, 0, (end_words - hdr_words) * 4, st));
  {
    uint64_t most = 0;
    for (uint32_t r = 0; r < n_bands; ++r) most = std::max<uint64_t>(most, meta[n_bands + r + 1] - meta[n_bands + r]);
    hipLaunchKernelGGL(enc_band_merge, dim3((uint32_t)((most + 4095) / 4096), n_bands), dim3(BAND_THREADS), 0, st,
                       (uint32_t*)d_out, d_words, dmeta, dmeta + n_bands, n_bands);
    hipLaunchKernelGGL(enc_band_fix, dim3(1), dim3(ENC_WAVE_THREADS), 0, st, d_out, d_words, dmeta + 2 * n_bands + 3,
                       dmeta + n_bands, n_bands, dmeta + 3 * n_bands + 3);
  }
  EncArgs a = ctx->bs.a;
  a.out = d_out;
  a.out_stride = 0;
  a.n_frames = 1;
  a.data_end = dmeta + 2 * n_bands + 1;
  a.out_len = dmeta + 2 * n_bands + 2;
  hipLaunchKernelGGL(enc_tail, grid_of(ctx->bs.plan.tail), dim3(ctx->bs.plan.tail.threads), 0, st, a);
  unsigned long long bad = 0;
  NICE_HIP(hipMemcpyAsync(&bad, dmeta + 3 * n_bands + 3, 8, hipMemcpyDeviceToHost, st));
  NICE_HIP(hipStreamSynchronize(st));   // `meta` lives on this stack frame
  if (bad) {   // a band was packed with a band_bits other than its own: its bits are missing
    *out_len = 0;
    return NICE_E_ARG;
  }
  *out_len = B + 5;
  NICE_HIP(hipGetLastError());
  return NICE_OK;
}

int nice_ctx_set_timing(nice_ctx* ctx, int on) {
  if (!ctx) return NICE_E_ARG;
  ctx->timer.on = on != 0;
  ctx->timer.marks.clear();
  ctx->timer.used = 0;
  return NICE_OK;
}

int nice_ctx_read_timing(nice_ctx* ctx, double* ms, uint32_t* count) {
  if (!ctx || !ms) return NICE_E_ARG;
  for (int i = 0; i < NICE_PHASES; ++i) {
    ms[i] = 0.0;
    if (count) count[i] = 0;
  }
  for (auto& m : ctx->timer.marks) {
    if (hipEventSynchronize(m.b) != hipSuccess) return NICE_E_HIP;
    float t = 0.f;
    if (hipEventElapsedTime(&t, m.a, m.b) != hipSuccess) return NICE_E_HIP;
    ms[m.phase] += t;
    if (count) count[m.phase] += 1;
  }
  ctx->timer.marks.clear();
  ctx->timer.used = 0;
  return NICE_OK;
}

// Test hook: the device heap replay (enc_tables) on n_vec host count vectors
// of n <= MAX_ALPHABET symbols; aob receives n_vec * n code lengths.
int nice_test_code_lengths(const uint32_t* counts, int n_vec, int n, uint8_t* aob) {
  if (n_vec <= 0 || n <= 0 || n > MAX_ALPHABET || !counts || !aob) return NICE_E_ARG;
  const size_t cb = (size_t)n_vec * n * 4, ab = (size_t)n_vec * n;
  void *dc = nullptr, *da = nullptr;
  NICE_HIP(hipMalloc(&dc, cb));
  if (hipMalloc(&da, ab) != hipSuccess) { (void)hipFree(dc); return NICE_E_HIP; }
  int rc = NICE_OK;
  if (hipMemcpy(dc, counts, cb, hipMemcpyHostToDevice) != hipSuccess) rc = NICE_E_HIP;
  if (!rc) {
    hipLaunchKernelGGL(enc_code_lengths_test, dim3(n_vec), dim3(ENC_WAVE_THREADS), 0, 0, (const uint32_t*)dc, n, (uint8_t*)da);
    if (hipGetLastError() != hipSuccess || hipMemcpy(aob, da, ab, hipMemcpyDeviceToHost) != hipSuccess)
      rc = NICE_E_HIP;
  }
  (void)hipFree(dc);
  (void)hipFree(da);
  return rc;
}

// Test hooks for dec_rows_split's fallback (tests/test_split.py).
// nice_test_occupy: `blocks` blocks of `lds_bytes` dynamic LDS each (one per
// CU at > 80 KB) on `stream`; blocks < short_blocks spin short_us, the others
// long_us (bounded busy waits on the real-time counter).
__global__ void nice_occupy_kernel(uint32_t short_blocks, unsigned long long short_ticks,
                                   unsigned long long long_ticks) {
  extern __shared__ uint32_t occ_lds[];
  if (threadIdx.x == 0) occ_lds[0] = blockIdx.x;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  const unsigned long long d = blockIdx.x < short_blocks ? short_ticks : long_ticks;
  while (__builtin_amdgcn_s_memrealtime() - t0 < d) __builtin_amdgcn_s_sleep(127);
}
int nice_test_occupy(void* stream, uint32_t blocks, uint32_t short_blocks, uint32_t short_us, uint32_t long_us,
                     uint32_t lds_bytes) {
  if (blocks == 0 || lds_bytes > LDS_BUDGET || long_us > 5000000 || short_us > 5000000) return NICE_E_ARG;
  NICE_HIP(hipFuncSetAttribute((const void*)nice_occupy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds_bytes));
  hipLaunchKernelGGL(nice_occupy_kernel, dim3(blocks), dim3(64), lds_bytes, (hipStream_t)stream, short_blocks,
                     (unsigned long long)short_us * 100ull, (unsigned long long)long_us * 100ull);
  NICE_HIP(hipGetLastError());
  return NICE_OK;
}
// The classify kernel the context's last encode (or band classify) used:
// 0 window, 1 tiny, 2 ring, 3 ring2 (32K ring), 4 strip, 5 pair (two tiles per iteration),
// 6 twin (per-tile row windows), 7 slide (per-lane sliding windows).
int nice_test_last_classify(nice_ctx* ctx) { return ctx ? ctx->last_classify : -1; }

// Test hooks of one context (tests only; nothing reads the environment for them):
// split_absent != 0 makes the last strip of every split decode return at entry
// (a strip that never became resident); pack_cap_bpp in [1, NICE_PACK_CAP_BPP]
// lowers enc_pack's LDS group buffer to that many bits per pixel (0: default).
int nice_test_set_hooks(nice_ctx* ctx, uint32_t split_absent, uint32_t pack_cap_bpp) {
  if (!ctx || pack_cap_bpp > NICE_PACK_CAP_BPP) return NICE_E_ARG;
  ctx->test_split_absent = split_absent ? 1u : 0u;
  ctx->test_pack_cap_bpp = pack_cap_bpp;
  return NICE_OK;
}

// Frames of the context's last split decode that went to the fallback launch
// (synchronises the device).
int nice_test_split_redos(nice_ctx* ctx, uint32_t* split_frames, uint32_t* redos) {
  if (!ctx || !redos || !split_frames) return NICE_E_ARG;
  *redos = 0;
  *split_frames = ctx->split_frames;
  if (!ctx->split_abort || !ctx->split_frames) return NICE_OK;
  NICE_HIP(hipSetDevice(ctx->device));
  NICE_HIP(hipDeviceSynchronize());
  std::vector<uint32_t> h(ctx->split_frames);
  NICE_HIP(hipMemcpy(h.data(), ctx->split_abort, h.size() * 4, hipMemcpyDeviceToHost));
  for (uint32_t v : h) *redos += v == SPLIT_REDO ? 1u : 0u;
  return NICE_OK;
}

// The row kernel the context's last decode launched and its redo launch, as
// DecRoute values (nice_dec_plan.hpp; 0: none).  ctx null: the context of the
// host-buffer entry points (nice_decode).
int nice_test_last_dec_route(nice_ctx* ctx, uint32_t* route, uint32_t* fallback) {
  if (!ctx) ctx = g_default;
  if (!ctx || !route || !fallback) return NICE_E_ARG;
  *route = ctx->last_dec_route;
  *fallback = ctx->last_dec_fallback;
  return NICE_OK;
}

int nice_test_last_tiled(nice_ctx* ctx, uint32_t* coded, uint32_t* raw) {
  if (!ctx || !coded || !raw) return NICE_E_ARG;
  *coded = ctx->last_tiled_coded;
  *raw = ctx->last_tiled_raw;
  return NICE_OK;
}

int nice_test_last_set(nice_ctx* ctx, uint32_t* coded, uint32_t* raw) {
  if (!ctx || !coded || !raw) return NICE_E_ARG;
  *coded = ctx->last_set_coded;
  *raw = ctx->last_set_raw;
  return NICE_OK;
}

int nice_test_last_set_merges(nice_ctx* ctx, uint32_t* launches) {
  if (!ctx || !launches) return NICE_E_ARG;
  *launches = ctx->last_set_merges;
  return NICE_OK;
}

int nice_test_last_set_alpha(nice_ctx* ctx, uint32_t* coded, uint32_t* raw, uint32_t* constant) {
  if (!ctx || !coded || !raw || !constant) return NICE_E_ARG;
  *coded = ctx->last_set_alpha_coded;
  *raw = ctx->last_set_alpha_raw;
  *constant = ctx->last_set_alpha_const;
  return NICE_OK;
}

int nice_test_set_option(int id, int64_t value) {
  if (id < 0 || id >= NICE_OPT_COUNT) return NICE_E_ARG;
  g_opt[id].store(value < 0 ? 0 : value + 1, std::memory_order_relaxed);
  return NICE_OK;
}

void nice_test_reset_options(void) {
  for (auto& o : g_opt) o.store(0, std::memory_order_relaxed);
}

const char* nice_phase_name(int phase) {
  return (phase >= 0 && phase < NICE_PHASES) ? kPhaseNames[phase] : "";
}

int nice_decode(const uint8_t* s, size_t len, uint8_t* px_out, size_t cap, uint32_t flags,
                size_t* px_len) {
  uint32_t w, h;
  uint8_t ch;
  int rc = nice_peek_header(s, len, &w, &h, &ch);
  if (rc) return rc;
  if (ch != 3 && ch != 4) return NICE_E_UNSUPPORTED;
  if ((flags & NICE_DEC_STRICT_REFERENCE) && ch != 3) return NICE_E_UNSUPPORTED;
  const uint64_t N = (uint64_t)w * h;
  if (N > (1ull << 30)) return NICE_E_ARG;
  if (px_len) *px_len = (size_t)N * ch;
  if (cap < N * ch || (N && !px_out)) return NICE_E_CAPACITY;
  nice_ctx* ctx;
  if ((rc = default_ctx(&ctx))) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  NICE_HIP(hipSetDevice(ctx->device));
  const size_t sbytes = align_up(len + 8, 256);
  const size_t pbytes = align_up((size_t)N * ch + 4, 256);
  if ((rc = ctx->host_out.grow(sbytes))) return rc;
  if ((rc = ctx->host_px.grow(pbytes))) return rc;
  if ((rc = ctx->dev_len.grow(256))) return rc;
  NICE_HIP(hipMemcpy(ctx->host_out.ptr, s, len, hipMemcpyHostToDevice));
  uint64_t l64 = len;
  NICE_HIP(hipMemcpy(ctx->dev_len.ptr, &l64, 8, hipMemcpyHostToDevice));
  int32_t* d_status = (int32_t*)((uint8_t*)ctx->dev_len.ptr + 64);
  rc = nice_decode_batch_dev(ctx, nullptr, (const uint8_t*)ctx->host_out.ptr, sbytes,
                             (const uint64_t*)ctx->dev_len.ptr, 1, w, h, ch,
                             (uint8_t*)ctx->host_px.ptr, pbytes, flags, d_status);
  if (rc) return rc;
  int32_t status = 0;
  NICE_HIP(hipMemcpy(&status, d_status, 4, hipMemcpyDeviceToHost));
  if (status) return status;
  if (N) NICE_HIP(hipMemcpy(px_out, ctx->host_px.ptr, (size_t)N * ch, hipMemcpyDeviceToHost));
  return NICE_OK;
}

}  // extern "C"
