// rows_host_check.cpp -- the barrier row kernels' body (dec_rows_body and its
// rows_* stages, csrc/nice_rows_body.hpp: the text the device compiles) on host
// threads, for tests/test_rows_host.py.  CPU only.
//   rows_host_check KERNEL W H OC[,OC..] SEED [SEED..] [left=0] [cover=0]
//     KERNEL  rows | rows8 | wide   (dec_rows, dec_rows8, dec_rows_wide)
//     OC      output channels, one per seed in turn
//     left=0  columns 0..2 take no record whose table index is negative in
//             ring slot 0 (classes 1..3 and 10..12, runs, stale slots): to
//             look past a known defect at what else a build does
//     cover=0 do not require the coverage condition below
// Per seed: random records in the format of nice_dec_rec.hpp (every class valid
// at the pixel, random constants, runs, stale-tag slots; chosen classes at the
// columns and first pixels below), the expected raster from a sequential loop
// with no ring, every buffer at exactly the planner's size (LDS, the global
// ring preset to a poison word, records, output), plan.rows.threads host
// threads through the body, then every output byte and the status compared.
// Coverage condition, over the seeds of one call: every cell (class, column,
// ring slot y & 3) on rows y >= 3 that is valid at this width has a record,
// for the columns {0, 1, 2, W-3, W-2, W-1}, the six columns around one interior
// segment edge (x mod 16 in 13..15, 0..2) and the first three of the last wave;
// and every class 1..13 is taken at the first three pixels at which its offset
// is valid (they reference pixels 0..2).  Seven consecutive seeds fill them.
// Prints one result line; exit 0 only without mismatch and with full coverage.
// Build: g++ -std=c++20 -O1 -g -fsanitize=address,undefined -pthread
//            -I tools/hip_host_shim -I <package>/csrc tools/rows_host_check.cpp
#include <hip/hip_runtime.h>   // tools/hip_host_shim: first, it renames glibc's nice()

#include <map>
#include <random>
#include <set>
#include <string>
#include <tuple>

#include "nice_dec_plan.hpp"
#include "nice_rows_body.hpp"

using namespace nice;

namespace {

constexpr uint32_t POISON = 0xDEADBEEFu;

template <class T>
T* exact_alloc(size_t bytes) {   // 16-byte aligned, not a byte more: the sanitizer sees every stray access
  void* p = nullptr;
  if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) abort();
  return static_cast<T*>(p);
}

struct Kernel {
  const char* name;
  DecRoute route;
  int seg;
  void (*body)(const DecArgs&);
};
const Kernel kKernels[] = {
    {"rows", DEC_R_ROWS, 16, [](const DecArgs& a) { dec_rows_body<ROWS_THREADS, true>(a); }},
    {"rows8", DEC_R_ROWS8, 8, [](const DecArgs& a) { dec_rows_body<ROWS_THREADS, true, 8>(a); }},
    {"wide", DEC_R_ROWS_WIDE, 16, [](const DecArgs& a) { dec_rows_body<ROWS_WIDE_THREADS, false>(a); }},
};

// the plan of one frame with the options that force the kernel (tests/test_rows_store.py)
DecPlan plan_for(const Kernel& k, uint32_t W, uint32_t H) {
  DecOpts o{};
  o.split = DecOpt{true, 0};
  if (k.route == DEC_R_ROWS) o.flow = DecOpt{true, 0};
  if (k.route == DEC_R_ROWS8) o.seg = DecOpt{true, 8};
  const uint64_t len = FILE_HEADER_BYTES + (TABLE_HEADER_BITS + 7) / 8 + (uint64_t)W * H;
  return plan_decode(DecShape{1, W, H, 256, len, (uint64_t)W * H * 8}, o);
}

int64_t cls_off(int c, uint32_t W) { return (int64_t)cls_rows(c) * W + cls_px(c); }
bool cls_valid(int c, uint64_t p, uint32_t W) { return c == 0 || (cls_off(c, W) > 0 && (uint64_t)cls_off(c, W) <= p); }
// left=0: a class whose table word lies before the referenced row's pixel 0
bool reaches_left(int c) { return cls_px(c) > 0; }

std::vector<uint32_t> special_columns(uint32_t W, int seg) {
  std::set<uint32_t> s{0, 1, 2, W - 3, W - 2, W - 1};
  const uint32_t wave = 64u * (uint32_t)seg;
  uint32_t e = 16 * ((W / 16) / 2);
  if (e % wave == 0) e += 16;
  for (uint32_t x = e - 3; x < e + 3; ++x) s.insert(x);
  if (W > wave) {
    const uint32_t wv = (W - 1) / wave * wave;
    for (uint32_t x = wv; x < wv + 3 && x < W; ++x) s.insert(x);
  }
  return std::vector<uint32_t>(s.begin(), s.end());
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: rows_host_check rows|rows8|wide W H OC[,OC..] SEED [SEED..] [left=0] [cover=0]\n");
    return 2;
  }
  const Kernel* K = nullptr;
  for (const Kernel& k : kKernels)
    if (!strcmp(argv[1], k.name)) K = &k;
  const uint32_t W = (uint32_t)atoll(argv[2]), H = (uint32_t)atoll(argv[3]);
  std::vector<uint32_t> ocs;
  for (const char* s = argv[4]; *s; s += strspn(s, ",")) {
    ocs.push_back((uint32_t)atoi(s));
    s += strcspn(s, ",");
  }
  std::vector<uint64_t> seeds;
  bool left = true, cover = true;
  for (int i = 5; i < argc; ++i) {
    if (!strcmp(argv[i], "left=0")) left = false;
    else if (!strcmp(argv[i], "cover=0")) cover = false;
    else seeds.push_back((uint64_t)atoll(argv[i]));
  }
  if (!K || W < 64 || H < 1 || seeds.empty() || ocs.empty()) { fprintf(stderr, "bad arguments\n"); return 2; }
  for (uint32_t oc : ocs)
    if (oc != 3 && oc != 4) { fprintf(stderr, "OC is 3 or 4\n"); return 2; }
  const DecPlan plan = plan_for(*K, W, H);
  if (plan.rows.route != K->route) {
    fprintf(stderr, "the planner does not send %u columns to %s (route %u)\n", W, K->name, (uint32_t)plan.rows.route);
    return 2;
  }
  const bool lds_ring = K->route != DEC_R_ROWS_WIDE;
  const uint32_t threads = plan.rows.threads;
  const size_t lds_bytes = rows_lds_bytes(threads, W, lds_ring);
  if (plan.rows.lds != lds_bytes) { fprintf(stderr, "plan LDS %zu, layout %zu\n", plan.rows.lds, lds_bytes); return 2; }
  const size_t ring_bytes = (size_t)ROWS_RING * rows_ring_stride(W) * 4;
  if (!lds_ring && plan.rowbuf != ring_bytes) { fprintf(stderr, "plan rowbuf %zu, ring %zu\n", plan.rowbuf, ring_bytes); return 2; }
  const uint64_t N = (uint64_t)W * H, rec_stride = (N + 3) & ~3ull;

  const std::vector<uint32_t> cols = special_columns(W, K->seg);
  std::map<std::tuple<int, uint32_t, uint32_t>, unsigned> cells;   // (class, column, slot) -> records, y >= 3
  std::map<std::pair<int, int>, unsigned> firsts;                  // (class, k): pixel off + k takes the class
  for (int c = 0; c < 14; ++c) {
    for (uint32_t x : cols)
      for (uint32_t y = 3; y < H; ++y)
        if (cls_valid(c, (uint64_t)y * W + x, W)) cells[{c, x, y & 3u}] += 0;
    for (int k = 0; k < 3 && c > 0; ++k)
      if ((uint64_t)cls_off(c, W) + k < N) firsts[{c, k}] += 0;
  }

  unsigned long long wrong = 0, first_wrong = ~0ull;
  int status_seen = 0;
  for (size_t si = 0; si < seeds.size(); ++si) {
    const uint64_t seed = seeds[si];
    const uint32_t OC = ocs[si % ocs.size()];
    std::mt19937_64 rng(seed * 0x9E3779B97F4A7C15ull + W);
    auto rnd = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    const uint32_t tag = 1 + rnd(15);
    const uint32_t flags = rnd(2) ? NICE_DEC_ALPHA_FILL_FF : 0u;

    // ---- records
    uint32_t* recs = exact_alloc<uint32_t>(rec_stride * 4);
    auto constant = [&] {
      uint32_t c = 0;
      for (int ch = 0; ch < 3; ++ch) c |= (rnd(4) ? rnd(256) : (rnd(2) ? 255u : 0u)) << (10 * ch);
      return c;
    };
    auto record = [&](int cls) { return (uint32_t)cls << 28 | constant() | rec_tagbits(tag); };
    auto any_class = [&](uint64_t p, bool no_left) {
      for (;;) {
        const int c = (int)rnd(14);
        if (cls_valid(c, p, W) && !(no_left && reaches_left(c))) return c;
      }
    };
    uint32_t run = 0;
    for (uint64_t p = 0; p < rec_stride; ++p) {
      const bool no_left = !left && p % W < 3;
      if (p >= N) recs[p] = (uint32_t)rng();   // the frame's alignment words: never read as pixels
      else if (run && !no_left) { recs[p] = REC_RUN | rec_tagbits(tag); --run; }
      else if (rnd(100) < 5 && !no_left) { recs[p] = REC_RUN | rec_tagbits(tag); run = rnd(8); }
      else if (rnd(100) < 3 && !no_left) {   // a stale slot: another call's tag, or a cleared word
        const uint32_t other = (tag + rnd(15)) % 15 + 1;
        recs[p] = rnd(3) ? (((uint32_t)rng() & ~REC_TAG_MASK) | rec_tagbits(other == tag ? 0 : other)) : 0u;
      } else recs[p] = record(any_class(p, no_left));
    }
    // the special columns, rows 4..: the classes in turn over seeds and ring turns
    for (size_t ci = 0; ci < cols.size(); ++ci)
      for (uint32_t y = 4; y < H; ++y) {
        const int c = (int)((2 * seed + ((y - 4) >> 2) + ci) % 14);
        const uint64_t p = (uint64_t)y * W + cols[ci];
        if (cls_valid(c, p, W) && !(!left && cols[ci] < 3 && reaches_left(c))) recs[p] = record(c);
      }
    // the first pixels at which each offset is valid, where several classes meet: one of them by seed
    {
      std::map<uint64_t, std::vector<int>> at;
      for (int c = 1; c < 14; ++c)
        for (int k = 0; k < 3; ++k) {
          const uint64_t p = (uint64_t)cls_off(c, W) + k;
          if (p < N && !(!left && p % W < 3 && reaches_left(c))) at[p].push_back(c);
        }
      for (const auto& [p, cs] : at) recs[p] = record(cs[(seed + p) % cs.size()]);
    }

    // ---- expected raster (no ring) and what the records cover
    std::vector<uint8_t> want(N * 3);
    for (uint64_t p = 0; p < N; ++p) {
      const uint32_t r = (recs[p] & REC_TAG_MASK) == rec_tagbits(tag) ? recs[p] : REC_RUN;
      const int cls = (int)(r >> 28);
      const uint32_t x = (uint32_t)(p % W), y = (uint32_t)(p / W);
      for (int ch = 0; ch < 3; ++ch) {
        const uint32_t c = (r >> (10 * ch)) & 0xFFu;
        auto px = [&](int64_t q) -> uint32_t { return q < 0 ? 0u : want[(uint64_t)q * 3 + ch]; };
        uint32_t v;
        if (cls == 0) v = y == 0 ? px((int64_t)p - 1) + c : ((px((int64_t)p - 1) + px((int64_t)p - W)) >> 1) + c;
        else v = px((int64_t)p - cls_off(cls, W)) + c;
        want[p * 3 + ch] = (uint8_t)v;
      }
      if (y >= 3) {
        auto it = cells.find({cls, x, y & 3u});
        if (it != cells.end()) ++it->second;
      }
      if (cls > 0 && (int64_t)p >= cls_off(cls, W) && (int64_t)p < cls_off(cls, W) + 3) ++firsts[{cls, (int)((int64_t)p - cls_off(cls, W))}];
    }

    // ---- the block
    uint32_t* lds = exact_alloc<uint32_t>(lds_bytes);
    memset(lds, 0xA5, lds_bytes);   // LDS holds whatever the last block left
    uint32_t* rowbuf = nullptr;
    if (!lds_ring) {
      rowbuf = exact_alloc<uint32_t>(ring_bytes);
      for (size_t i = 0; i < ring_bytes / 4; ++i) rowbuf[i] = POISON;
    }
    uint8_t* out = exact_alloc<uint8_t>(N * OC);
    memset(out, 0x5A, N * OC);
    int32_t* status = exact_alloc<int32_t>(4);
    *status = 0;
    DecArgs a{};
    a.n_frames = 1; a.W = W; a.H = H;
    a.out_channels = OC; a.flags = flags;
    a.px_out = out; a.px_stride = N * OC;
    a.status = status;
    a.recs = recs; a.rec_stride = rec_stride; a.rec_tag = tag;
    a.rows_in_lds = lds_ring; a.rowbuf = rowbuf;
    hip_host_shim::launch(K->body, a, threads, lds);

    // ---- compare
    const uint8_t alpha = flags ? 255 : 0;
    for (uint64_t p = 0; p < N; ++p) {
      bool ok = !memcmp(out + p * OC, &want[p * 3], 3) && (OC == 3 || out[p * 4 + 3] == alpha);
      if (!ok) {
        ++wrong;
        if (first_wrong == ~0ull) {
          first_wrong = p;
          fprintf(stderr, "seed %llu OC %u: pixel %llu (row %llu, column %llu; 3W-1 = %llu) class %u: got %u %u %u, want %u %u %u\n",
                  (unsigned long long)seed, OC, (unsigned long long)p, (unsigned long long)(p / W), (unsigned long long)(p % W),
                  3ull * W - 1, rec_canon(recs[p], tag) >> 28, out[p * OC], out[p * OC + 1], out[p * OC + 2], want[p * 3],
                  want[p * 3 + 1], want[p * 3 + 2]);
        }
      }
    }
    if (*status != 0 && !status_seen) status_seen = *status;
    free(recs); free(lds); free(rowbuf); free(out); free(status);
  }

  unsigned empty = 0;
  for (const auto& [cell, n] : cells)
    if (!n) {
      if (cover && empty++ < 8)
        fprintf(stderr, "no record: class %d column %u slot %u\n", std::get<0>(cell), std::get<1>(cell), std::get<2>(cell));
    }
  for (const auto& [cell, n] : firsts)
    if (!n) {
      if (cover && empty++ < 8) fprintf(stderr, "no record: class %d at its first valid pixel + %d\n", cell.first, cell.second);
    }
  const bool ok = wrong == 0 && status_seen == 0 && empty == 0;
  printf("rows_host_check kernel=%s W=%u H=%u threads=%u seeds=%zu wrong_pixels=%llu status=%d cells=%zu empty_cells=%u%s %s\n",
         K->name, W, H, threads, seeds.size(), wrong, status_seen, cells.size() + firsts.size(), empty,
         cover ? "" : " (coverage not required)", ok ? "OK" : "FAIL");
  return ok ? 0 : 1;
}
