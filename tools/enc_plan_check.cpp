// enc_plan_check.cpp -- the encoder's launch planner (csrc/nice_enc_plan.hpp)
// on the CPU, for tests/test_enc_plan.py and tests/test_classify_routes.py:
//   enc_plan_check plan W H C N_FRAMES CUS [al4=V] [al16=V] [band=LO:HI] [no_ring=V] [no_pair=V] [no_slide=V]
//                          one plan as a line of key=value fields (16-byte aligned frames and no
//                          options unless given; band: tiles [LO, HI) of one image, N_FRAMES = 1)
//   enc_plan_check sweep   every W in 1..20000 x channels {3, 4} x heights {1, 8, 2160} x the three
//                          alignments, for batches of {1, 2, 64, 512} frames and for a few bands of
//                          one image, at 256 CUs: every plan is launchable and legal for its shape;
//                          prints the violations and the count
// Build: g++ -O2 -std=c++17 -I <package>/csrc tools/enc_plan_check.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "nice_enc_plan.hpp"

using namespace nice;

static const char* kKind[] = {"window", "tiny", "ring", "ring2", "strip", "pair", "twin", "slide"};

// The __global__ entry a plan names (csrc/nice_kernels.h).
static std::string kernel_name(const EncPlan& p) {
  static const char* base[][2] = {{"enc_classify", "enc_classify"}, {"enc_classify_tiny", "enc_classify_tiny"},
                                  {"enc_classify_ring", "enc_classify_ring3"},
                                  {"enc_classify_ring2", "enc_classify_ring2_3"}, {"enc_classify_strip", ""},
                                  {"enc_classify_pair", ""}, {"enc_classify_twin", "enc_classify_twin3"},
                                  {"enc_classify_slide", ""}};
  std::string n = base[p.kind][p.rgb ? 1 : 0];
  if (p.kind == CLS_K_SLIDE) return n + std::to_string(p.wmod4);
  const bool staged = p.kind != CLS_K_WINDOW && p.kind != CLS_K_TINY;
  return n + (staged && p.flags_out ? "_m" : "");
}

static EncShape shape(uint32_t w, uint32_t h, int c, uint32_t n_frames, int cus, bool al4, bool al16) {
  EncShape s{};
  s.n_frames = n_frames;
  s.w = w;
  s.h = h;
  s.channels = (uint8_t)c;
  s.cus = cus;
  s.aligned4 = al4;
  s.aligned16 = al16;
  return s;
}

// Launch limits: grid x < 2^31, grid y < 2^16; the block size is the kernel's.
static bool grid_ok(const EncLaunch& l, int threads) {
  return l.x >= 1 && l.x <= 0x7FFFFFFFu && l.y >= 1 && l.y <= 65535u && l.threads == (uint32_t)threads;
}

// What the kernels and the hardware need of a plan; 0 when it holds.
//   1 kind   2 coverage   4 ring clamps   8 strip rows   16 grids / block sizes   32 run digits   64 pack
static int check(const EncShape& s, const EncPlan& p) {
  int bad = 0;
  const uint32_t w = s.w, nt = p.tile_hi - p.tile_lo;
  const uint64_t work = (uint64_t)s.n_frames * nt;
  const bool rgba = s.channels == 4;
  const ClsKind k = p.kind;
  const bool ring = k == CLS_K_RING || k == CLS_K_RING2 || k == CLS_K_PAIR || k == CLS_K_SLIDE;
  const bool staged = k != CLS_K_WINDOW && k != CLS_K_TINY;
  // kind
  if ((k == CLS_K_TINY) != (w < 3)) bad |= 1;
  if ((k == CLS_K_WINDOW) != (w >= 3 && !s.aligned4)) bad |= 1;
  if ((k == CLS_K_SLIDE || k == CLS_K_PAIR) && !(rgba && w <= CLS_PAIR_MAX_W)) bad |= 1;
  if (k == CLS_K_SLIDE && !(s.aligned16 && !s.band)) bad |= 1;
  if (k == CLS_K_RING && w > CLS_RING_MAX_W) bad |= 1;
  if (k == CLS_K_STRIP && !(rgba && w % ENC_TILE == 0)) bad |= 1;
  if (k == CLS_K_RING2 && w > CLS_RING2_MAX_W) bad |= 1;
  if (p.rgb != !rgba || p.wmod4 != (w & 3u) || kernel_name(p).empty() || p.flags_out != (staged && !s.band)) bad |= 1;
  // coverage: the blocks' shares cover the work and no block is empty
  const uint64_t blocks = p.classify.x, per = p.tiles_per_block;
  if (k == CLS_K_STRIP) {
    const uint32_t tpr = w / ENC_TILE;
    const uint64_t rows = s.band ? (p.tile_hi + tpr - 1) / tpr - p.tile_lo / tpr : s.h;
    const uint64_t strips = (w + STRIP_W - 1) / STRIP_W;
    if (per < 1 || per > rows) bad |= 8;
    else if (blocks != s.n_frames * strips * ((rows + per - 1) / per) || ((rows + per - 1) / per - 1) * per >= rows) bad |= 2;
  } else if (per < 1 || blocks * per < work || (blocks - 1) * per >= work) {
    bad |= 2;
  }
  if (ring && (per < 16 || per > 16384)) bad |= 4;
  // grids and block sizes
  if (!grid_ok(p.classify, staged ? CLS_THREADS : ENC_THREADS)) bad |= 16;
  if (p.rundigits.on() && !grid_ok(p.rundigits, RUNDIGITS_THREADS)) bad |= 16;
  if (p.groups != (nt + ENC_GROUP_TILES - 1) / ENC_GROUP_TILES || p.group_reduce.on() != (p.groups > 1)) bad |= 16;
  if (p.group_reduce.on() && !grid_ok(p.group_reduce, GROUP_THREADS)) bad |= 16;
  if (!grid_ok(p.tailruns, TR_THREADS) || !grid_ok(p.tilescan, SCAN_THREADS)) bad |= 16;
  if (p.tailruns.x != p.groups || p.tilescan.x != p.groups || p.tailruns.y != s.n_frames || p.tilescan.y != s.n_frames) bad |= 16;
  if (!grid_ok(p.tables, ENC_WAVE_THREADS) || !grid_ok(p.header, ENC_WAVE_THREADS) || !grid_ok(p.tail, ENC_WAVE_THREADS)) bad |= 16;
  if (!grid_ok(p.packtab, PACKTAB_THREADS) || !grid_ok(p.long_path, ENC_THREADS)) bad |= 16;
  if (!grid_ok(p.pack, PK_THREADS) || !grid_ok(p.pack_over, PK_THREADS) || !grid_ok(p.edges, EDGES_THREADS)) bad |= 16;
  if ((uint64_t)p.tail.x * ENC_WAVE_THREADS < s.n_frames) bad |= 16;
  // run digits from the coded flags: frames of the staged kernels
  if (p.rundigits.on() != (!s.band && staged) || p.cmask_std != (p.rundigits.on() ? 1u : 0u)) bad |= 32;
  if ((p.il == 1) != (k == CLS_K_SLIDE) || (p.rundigits.on() && p.rundigits.y != s.n_frames)) bad |= 32;
  // pack: a persistent grid, every slot with at least one block
  if (p.pack.x > (uint64_t)s.cus * PACK_BLOCKS_PER_CU || p.pack.x > work) bad |= 64;
  if (p.pack_slots < 1 || p.pack_slots > 64 || p.pack_slots > s.n_frames) bad |= 64;
  return bad;
}

static void print_plan(const EncPlan& p) {
  printf("kind=%s kind_id=%d kernel=%s rgb=%d flags_out=%d wmod4=%u cls_x=%u cls_y=%u cls_threads=%u tiles_per_block=%u "
         "rd_x=%u rd_y=%u rd_threads=%u il=%d cmask_std=%u groups=%u gr_x=%u gr_y=%u tr_x=%u tr_y=%u ts_x=%u ts_y=%u "
         "tables_x=%u header_x=%u packtab_x=%u long_x=%u pack_x=%u pack_slots=%u over_x=%u edges_x=%u edges_y=%u "
         "tail_x=%u tiles=%u tile_lo=%u tile_hi=%u\n",
         kKind[p.kind], (int)p.kind, kernel_name(p).c_str(), p.rgb ? 1 : 0, p.flags_out ? 1 : 0, p.wmod4, p.classify.x,
         p.classify.y, p.classify.threads, p.tiles_per_block, p.rundigits.x, p.rundigits.y, p.rundigits.threads, p.il,
         p.cmask_std, p.groups, p.group_reduce.x, p.group_reduce.y, p.tailruns.x, p.tailruns.y, p.tilescan.x,
         p.tilescan.y, p.tables.x, p.header.x, p.packtab.x, p.long_path.x, p.pack.x, p.pack_slots, p.pack_over.x,
         p.edges.x, p.edges.y, p.tail.x, p.tiles_per_frame, p.tile_lo, p.tile_hi);
}

int main(int argc, char** argv) {
  if (argc >= 7 && !strcmp(argv[1], "plan")) {
    EncShape s = shape((uint32_t)atoll(argv[2]), (uint32_t)atoll(argv[3]), atoi(argv[4]), (uint32_t)atoll(argv[5]),
                       atoi(argv[6]), true, true);
    EncOpts o{};
    const struct { const char* key; bool* v; } keys[] = {{"al4=", &s.aligned4}, {"al16=", &s.aligned16},
                                                         {"no_ring=", &o.no_ring}, {"no_pair=", &o.no_pair},
                                                         {"no_slide=", &o.no_slide}};
    for (int i = 7; i < argc; ++i) {
      bool known = false;
      for (const auto& k : keys)
        if (!strncmp(argv[i], k.key, strlen(k.key))) {
          *k.v = atoll(argv[i] + strlen(k.key)) != 0;
          known = true;
        }
      unsigned lo, hi;
      if (!known && sscanf(argv[i], "band=%u:%u", &lo, &hi) == 2) {
        s.band = true;
        s.tile_lo = lo;
        s.tile_hi = hi;
        known = true;
      }
      if (!known) { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if ((s.channels != 3 && s.channels != 4) ||
        (s.band && (s.n_frames != 1 || s.tile_lo >= s.tile_hi || s.tile_hi > enc_tiles(s.w, s.h)))) {
      fprintf(stderr, "bad shape\n");
      return 2;
    }
    print_plan(plan_encode(s, o));
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "sweep")) {
    const uint32_t frames[] = {1, 2, 64, 512}, heights[] = {1, 8, 2160};
    const bool align[][2] = {{false, false}, {true, false}, {true, true}};   // 4-byte, 16-byte
    unsigned long long n = 0, bad = 0;
    auto one = [&](const EncShape& s) {
      const EncPlan p = plan_encode(s, EncOpts{});
      ++n;
      const int b = check(s, p);
      if (b) {
        ++bad;
        if (bad <= 200)
          printf("violation w=%u h=%u c=%d n_frames=%u al4=%d al16=%d band=%d:%u:%u mask=0x%x kind=%s\n", s.w, s.h,
                 s.channels, s.n_frames, s.aligned4, s.aligned16, s.band, s.tile_lo, s.tile_hi, b, kKind[p.kind]);
      }
    };
    for (uint32_t w = 1; w <= 20000; ++w)
      for (int c = 3; c <= 4; ++c)
        for (uint32_t h : heights)
          for (const auto& al : align) {
            for (uint32_t nf : frames) one(shape(w, h, c, nf, 256, al[0], al[1]));
            // bands of one image: all of it, its first tile, its last third, its last tile
            const uint32_t T = enc_tiles(w, h);
            const uint32_t bands[][2] = {{0, T}, {0, 1}, {T - (T + 2) / 3, T}, {T - 1, T}};
            for (const auto& b : bands) {
              EncShape s = shape(w, h, c, 1, 256, al[0], al[1]);
              s.band = true;
              s.tile_lo = b[0];
              s.tile_hi = b[1];
              one(s);
            }
          }
    printf("checked %llu plans, %llu violations\n", n, bad);
    return bad ? 1 : 0;
  }
  fprintf(stderr, "usage: %s plan W H C N_FRAMES CUS [opt=V ...] | sweep\n", argv[0]);
  return 2;
}
