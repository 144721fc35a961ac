// dec_plan_check.cpp -- the decoder's launch planner (csrc/nice_dec_plan.hpp)
// on the CPU, for tests/test_dec_plan.py and tests/test_dec_route.py:
//   dec_plan_check plan W H N_FRAMES CUS [single_wave=V] [seg=V] [split=V] [flow=V]
//                                          one plan (options unset unless given) as a line of key=value fields
//   dec_plan_check sweep                   every W in 1..40000 x the batch sizes below at 256 CUs: each plan
//                                          is launchable, or refused (route none: rows too wide for any
//                                          kernel); prints the violations and both counts
// Build: g++ -O2 -std=c++17 -I <package>/csrc tools/dec_plan_check.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nice_dec_plan.hpp"

using namespace nice;

static const char* kRoute[] = {"none", "dec_reconstruct", "dec_rows", "dec_rows8", "dec_rows_wide", "dec_rows_flow",
                               "dec_rows_split"};

static DecPlan plan(uint32_t w, uint32_t h, uint32_t n_frames, int cus, const DecOpts& o = DecOpts{}) {
  const uint64_t len = FILE_HEADER_BYTES + (TABLE_HEADER_BITS + 7) / 8 + (uint64_t)w * h;   // ~8 bits per pixel
  const uint64_t bits = (uint64_t)w * h * 8 * n_frames;
  return plan_decode(DecShape{n_frames, w, h, cus, len, bits}, o);
}

// What the hardware and the kernels need of a launch; 0 when it holds.
static int check_launch(const DecPlan& p, const DecLaunch& l, uint32_t w) {
  int bad = 0;
  if (l.lds + 1024 > LDS_BUDGET) bad |= 1;                   // dynamic + static LDS
  if (l.threads == 0 || l.threads % 64 || l.threads > dec_route_max_threads(l.route)) bad |= 2;
  const uint32_t nseg = (w + ROWS_SEG - 1) / ROWS_SEG, wpr = (nseg + 63) / 64;
  if (l.route == DEC_R_SPLIT) {
    const uint32_t sps = p.strips ? (nseg + p.strips - 1) / p.strips : 0;
    for (uint32_t j = 0; j < p.strips; ++j) {   // the kernel's own strip bounds
      const uint32_t s0 = j * sps, s1 = nseg < s0 + sps ? nseg : s0 + sps;
      if (s1 < s0 + 2 || s1 - s0 > SPLIT_THREADS) bad |= 4;
    }
    if (p.strips < 2 || p.split_frames < 1 || l.lds < split_lds_bytes(sps * ROWS_SEG)) bad |= 4;
  }
  if (l.route == DEC_R_FLOW) {
    if (p.flow_k < 1 || p.flow_k > 4 || p.flow_k * wpr > FLOW_THREADS / 64 || l.threads != 64 * p.flow_k * wpr) bad |= 8;
    if ((p.flow_ring != 4 && p.flow_ring != 8) || p.flow_k + 3 > p.flow_ring) bad |= 8;   // rows y-3..y-1 and k in flight
    if (l.lds != flow_lds_bytes(p.flow_ring, w)) bad |= 8;
  }
  return bad;
}

int main(int argc, char** argv) {
  if (argc >= 6 && !strcmp(argv[1], "plan")) {
    DecOpts o{};
    const struct { const char* key; DecOpt* opt; } keys[] = {
        {"single_wave=", &o.single_wave}, {"seg=", &o.seg}, {"split=", &o.split}, {"flow=", &o.flow}};
    for (int i = 6; i < argc; ++i) {
      bool known = false;
      for (const auto& k : keys)
        if (!strncmp(argv[i], k.key, strlen(k.key))) {
          *k.opt = DecOpt{true, atoll(argv[i] + strlen(k.key))};
          known = true;
        }
      if (!known) { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    const uint32_t w = (uint32_t)atoll(argv[2]);
    const DecPlan p = plan(w, (uint32_t)atoll(argv[3]), (uint32_t)atoll(argv[4]), atoi(argv[5]), o);
    printf("route=%s threads=%u lds=%zu fallback=%s fb_threads=%u fb_lds=%zu strips=%u split_frames=%u flow_k=%u "
           "flow_ring=%u route_id=%u fallback_id=%u\n", kRoute[p.rows.route], p.rows.threads, p.rows.lds,
           kRoute[p.fallback.route], p.fallback.threads, p.fallback.lds, p.strips, p.split_frames, p.flow_k,
           p.flow_ring, (uint32_t)p.rows.route, (uint32_t)p.fallback.route);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "sweep")) {
    const uint32_t frames[] = {1, 2, 64, 128, 129, 256, 257, 512};
    unsigned long long n = 0, bad = 0, refused = 0;
    uint32_t refused_from = 0;
    for (uint32_t nf : frames)
      for (uint32_t w = 1; w <= 40000; ++w) {
        const DecPlan p = plan(w, 8, nf, 256);
        ++n;
        if (p.rows.route == DEC_R_NONE) {
          if (!refused++ || w < refused_from) refused_from = w;
          continue;
        }
        int b = check_launch(p, p.rows, w);
        if (p.fallback.route != DEC_R_NONE) b |= check_launch(p, p.fallback, w) << 8;
        if (b) {
          ++bad;
          printf("violation w=%u n_frames=%u mask=0x%x route=%s threads=%u lds=%zu fallback=%s fb_threads=%u fb_lds=%zu\n",
                 w, nf, b, kRoute[p.rows.route], p.rows.threads, p.rows.lds, kRoute[p.fallback.route],
                 p.fallback.threads, p.fallback.lds);
        }
      }
    printf("checked %llu plans, %llu violations, %llu refused from w=%u\n", n, bad, refused, refused_from);
    return bad ? 1 : 0;
  }
  fprintf(stderr, "usage: %s plan W H N_FRAMES CUS [opt=V ...] | sweep\n", argv[0]);
  return 2;
}
