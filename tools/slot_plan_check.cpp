// slot_plan_check.cpp -- the slot planner of the tiled and set decodes
// (csrc/nice_slot_plan.hpp) on the CPU, for tests/test_slot_plan.py:
//   slot_plan_check sweep   one-image sets: every (width 1..40, tile width 2..9, window columns) joined
//                           with 8 of the same cases for the rows, so that every case occurs 8 times on
//                           either axis; then 20000 three-image sets of up to four windows, repeats and
//                           overlaps included, from a fixed seed.  Both planners on every one, against a
//                           brute-force list of the tiles each window overlaps; prints the violations
//                           and "checked N plans, V violations"
//   slot_plan_check rules   one literal table of tile entries through both rule lists, boundaries
//                           included, and the tiled case against the one-image, one-window set
// Build: g++ -O2 -std=c++17 -I <package>/csrc tools/slot_plan_check.cpp
#include <stdio.h>
#include <string.h>

#include <vector>

#include "nice_slot_plan.hpp"

using namespace nice;

namespace {

struct Win { uint32_t img, x0, y0, rw, rh; };
struct RefSlot { uint32_t win, ti, gt; };

// The slots by brute force: a tile is a slot of a window iff the rectangles
// overlap; windows in order, tiles in raster order.  Also: the tiles, cut to
// the window, cover each of its pixels exactly once.
bool ref_slots(const std::vector<uint32_t>& w, const std::vector<uint32_t>& h, uint32_t tw, uint32_t th,
               const std::vector<Win>& wins, std::vector<RefSlot>& out, std::vector<uint32_t>& slot_first) {
  bool ok = true;
  std::vector<uint32_t> first(w.size() + 1, 0);
  for (size_t i = 0; i < w.size(); ++i) first[i + 1] = first[i] + ((w[i] + tw - 1) / tw) * ((h[i] + th - 1) / th);
  std::vector<uint8_t> seen;
  for (uint32_t j = 0; j < wins.size(); ++j) {
    const Win& q = wins[j];
    const uint32_t nx = (w[q.img] + tw - 1) / tw, ny = (h[q.img] + th - 1) / th;
    slot_first.push_back((uint32_t)out.size());
    seen.assign((size_t)q.rw * q.rh, 0);
    for (uint32_t ty = 0; ty < ny; ++ty)
      for (uint32_t tx = 0; tx < nx; ++tx) {
        const uint32_t ax = tx * tw, ay = ty * th;
        if (ax >= q.x0 + q.rw || ax + tw <= q.x0 || ay >= q.y0 + q.rh || ay + th <= q.y0) continue;
        out.push_back({j, ty * nx + tx, first[q.img] + ty * nx + tx});
        for (uint32_t y = ay; y < ay + th; ++y)
          for (uint32_t x = ax; x < ax + tw; ++x)
            if (x >= q.x0 && x < q.x0 + q.rw && y >= q.y0 && y < q.y0 + q.rh) ++seen[(size_t)(y - q.y0) * q.rw + (x - q.x0)];
      }
    for (uint8_t s : seen) ok &= s == 1;
  }
  slot_first.push_back((uint32_t)out.size());
  return ok;
}

// The packer: the columns hold the plan's vectors, in order, disjoint, each
// naturally aligned; the statuses' tail 16-byte aligned behind them.
bool table_ok(const SlotPlan& p, const void* head, size_t head_bytes) {
  SlotTable t;
  pack_slot_table(p, head, head_bytes, t);
  struct Col { size_t off, bytes, elem; const void* data; };
  const Col cols[] = {{t.c_off, 8 * p.c_off.size(), 8, p.c_off.data()}, {t.c_len, 8 * p.c_len.size(), 8, p.c_len.data()},
                      {t.s_src, 8 * p.s_src.size(), 8, p.s_src.data()}, {t.c_idx, 4 * p.c_idx.size(), 4, p.c_idx.data()},
                      {t.c_win, 4 * p.c_win.size(), 4, p.c_win.data()}, {t.c_pos, 4 * p.c_pos.size(), 4, p.c_pos.data()},
                      {t.s_idx, 4 * p.s_idx.size(), 4, p.s_idx.data()}, {t.s_win, 4 * p.s_win.size(), 4, p.s_win.data()},
                      {t.s_kind, p.s_kind.size(), 1, p.s_kind.data()}};
  bool ok = head_bytes == 0 || !memcmp(t.host.data(), head, head_bytes);
  size_t end = head_bytes;
  for (const Col& c : cols) {
    ok &= c.off >= end && c.off % c.elem == 0 && c.off + c.bytes <= t.host.size();
    ok &= c.bytes == 0 || !memcmp(&t.host[c.off], c.data, c.bytes);
    end = c.off + c.bytes;
  }
  return ok && t.c_st >= end && t.c_st < end + 16 && t.c_st % 16 == 0 && t.host.size() == t.c_st &&
         t.bytes == t.c_st + 4 * p.c_off.size();
}

// One plan against the reference list.  alpha: every accepted slot is in the s
// columns and a coded one also in the c columns; colour: a slot is in one of them.
//   1 slot count   2 order / positions / windows / tile indices   4 not exactly one class   8 tile outside its image
//   16 columns of different lengths   32 counts by kind   64 packer
int check_plan(const SlotPlan& p, bool alpha, const std::vector<RefSlot>& ref, const SlotTables& t,
               const std::vector<uint32_t>& tiles_of_win, const void* head, size_t head_bytes) {
  int bad = 0;
  const size_t nc = p.c_off.size(), ns = p.s_src.size();
  if (p.init.size() != ref.size()) return 1;
  if (p.c_len.size() != nc || p.c_pos.size() != nc || p.s_idx.size() != ns || p.s_win.size() != ns) bad |= 16;
  if (alpha ? (p.s_kind.size() != ns || !p.c_idx.empty() || !p.c_win.empty())
            : (!p.s_kind.empty() || p.c_idx.size() != nc || p.c_win.size() != nc))
    bad |= 16;
  if (bad) return bad;
  size_t ic = 0, is = 0;
  uint32_t by_kind[3] = {0, 0, 0};
  for (uint32_t pos = 0; pos < ref.size(); ++pos) {
    const RefSlot& r = ref[pos];
    const uint8_t k = t.kind[r.gt];
    const bool refused = p.init[pos] != NICE_OK;
    const bool coded = ic < nc && p.c_pos[ic] == pos;
    const bool src = is < ns && p.s_idx[is] == r.ti && p.s_win[is] == r.win && (!alpha || p.s_kind[is] == k);
    if (refused) {
      if (coded) bad |= 4;
      continue;   // (an s entry that belongs to this slot is one too many: the walk ends with is != ns or a mismatch)
    }
    if (k > 2) { bad |= 4; continue; }
    ++by_kind[k];
    if (coded != (k == 0)) bad |= 4;
    if (coded) {
      if (p.c_off[ic] != t.off[r.gt] || p.c_len[ic] != t.len[r.gt]) bad |= 2;
      if (!alpha && (p.c_idx[ic] != r.ti || p.c_win[ic] != r.win)) bad |= 2;
      if (alpha && (!src || p.s_src[is] != ic)) bad |= 2;
      ++ic;
    }
    if (alpha || !coded) {
      if (!src) { bad |= 2; continue; }
      if (r.ti >= tiles_of_win[r.win]) bad |= 8;
      if (k == 1 && p.s_src[is] != t.off[r.gt]) bad |= 2;
      if (k == 2 && p.s_src[is] != t.val[r.gt]) bad |= 2;
      ++is;
    } else if (r.ti >= tiles_of_win[r.win]) {
      bad |= 8;
    }
  }
  if (ic != nc || is != ns) bad |= 4;
  if (memcmp(by_kind, p.by_kind, sizeof by_kind)) bad |= 32;
  if (!table_ok(p, head, head_bytes)) bad |= 64;
  return bad;
}

struct Lcg {
  uint64_t s;
  uint32_t next(uint32_t n) {   // 0 .. n-1
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((s >> 33) % n);
  }
};

unsigned long long g_plans = 0, g_bad = 0;

// Both planners on one set and its windows, over tables drawn from `rng`:
// every kind, sound and damaged offsets and lengths.
void check_case(const std::vector<uint32_t>& w, const std::vector<uint32_t>& h, uint32_t tw, uint32_t th,
                const std::vector<Win>& wins, Lcg& rng) {
  const uint32_t K = (uint32_t)w.size(), M = (uint32_t)wins.size();
  const uint64_t npx = (uint64_t)tw * th, bytes = 4096;
  std::vector<uint32_t> flat, first, nx, slot_first(M + 1), ref_first, tiles_of_win;
  for (const Win& q : wins) flat.insert(flat.end(), {q.img, q.x0, q.y0, q.rw, q.rh});
  int mask = 0;
  if (set_select(w.data(), h.data(), K, tw, th, flat.data(), M, first, nx, slot_first.data()) != NICE_OK) mask |= 1;
  std::vector<RefSlot> ref;
  if (!ref_slots(w, h, tw, th, wins, ref, ref_first)) mask |= 2;
  if (!mask && ref_first != slot_first) mask |= 1;
  if (!mask) {
    for (const Win& q : wins) tiles_of_win.push_back(first[q.img + 1] - first[q.img]);
    const uint32_t n = first[K];
    std::vector<uint64_t> off(n), len(n);
    std::vector<uint8_t> kind(n), val(n);
    static const uint8_t kinds[] = {0, 0, 0, 1, 1, 2, 2, 3, 7};
    for (uint32_t t = 0; t < n; ++t) {
      const uint64_t lens[] = {0, npx, 3 * npx, 17, bytes};
      kind[t] = kinds[rng.next(9)];
      off[t] = 16ull * rng.next(50) + (rng.next(8) == 0 ? 8 : 0) + (rng.next(16) == 0 ? bytes : 0);
      len[t] = lens[rng.next(5)];
      val[t] = (uint8_t)rng.next(256);
    }
    const SlotTables tabs{off.data(), len.data(), kind.data(), val.data(), bytes};
    const SlotWindows g{tw, th, first.data(), nx.data(), flat.data(), M, true};
    std::vector<uint64_t> head(3 * M, 0x0123456789abcdefull);   // stands for the window descriptors
    SlotPlan c, a;
    plan_colour_slots(tabs, g, c);
    plan_alpha_slots(tabs, g, a);
    mask |= check_plan(c, false, ref, tabs, tiles_of_win, head.data(), 8 * head.size());
    mask |= check_plan(a, true, ref, tabs, tiles_of_win, head.data(), 8 * head.size()) << 8;
  }
  g_plans += 2;
  if (mask) {
    ++g_bad;
    if (g_bad <= 100) {
      printf("violation mask=0x%x tile=%ux%u images", mask, tw, th);
      for (uint32_t i = 0; i < K; ++i) printf(" %ux%u", w[i], h[i]);
      for (const Win& q : wins) printf(" win=%u:%u,%u,%u,%u", q.img, q.x0, q.y0, q.rw, q.rh);
      printf("\n");
    }
  }
}

int sweep() {
  Lcg rng{2024};
  // one axis: every (image extent, tile extent, window start, window extent)
  struct Axis { uint32_t size, tile, lo, len; };
  std::vector<Axis> ax;
  for (uint32_t size = 1; size <= 40; ++size)
    for (uint32_t tile = 2; tile <= 9; ++tile)
      for (uint32_t lo = 0; lo < size; ++lo)
        for (uint32_t len = 1; lo + len <= size; ++len) ax.push_back({size, tile, lo, len});
  const size_t n = ax.size();   // 91840 = 2^6 * 5 * 7 * 41: 9973 is coprime to it
  for (size_t k = 0; k < 8; ++k)
    for (size_t i = 0; i < n; ++i) {
      const Axis &x = ax[i], &y = ax[(i * 9973 + k * 11479) % n];
      check_case({x.size}, {y.size}, x.tile, y.tile, {{0, x.lo, y.lo, x.len, y.len}}, rng);
    }
  for (int s = 0; s < 20000; ++s) {
    std::vector<uint32_t> w, h;
    for (int i = 0; i < 3; ++i) {
      w.push_back(1 + rng.next(40));
      h.push_back(1 + rng.next(40));
    }
    const uint32_t tw = 2 + rng.next(8), th = 2 + rng.next(8), M = 1 + rng.next(4);
    std::vector<Win> wins;
    for (uint32_t j = 0; j < M; ++j) {
      if (j && rng.next(4) == 0) {   // a repeat
        wins.push_back(wins[rng.next(j)]);
        continue;
      }
      Win q;
      q.img = rng.next(3);
      q.x0 = rng.next(w[q.img]);
      q.y0 = rng.next(h[q.img]);
      q.rw = 1 + rng.next(w[q.img] - q.x0);
      q.rh = 1 + rng.next(h[q.img] - q.y0);
      wins.push_back(q);
    }
    check_case(w, h, tw, th, wins, rng);
  }
  printf("checked %llu plans, %llu violations\n", g_plans, g_bad);
  return g_bad ? 1 : 0;
}

// ---- rules ---------------------------------------------------------------------
// Tiles of 4 x 4 pixels (a raw colour tile is 48 bytes, a raw alpha plane 16)
// in a batch of 256 bytes.  What each planner makes of the entry: C coded,
// R raw / sourced, F NICE_E_FORMAT, A NICE_E_ARG.
struct Rule { uint8_t kind; uint64_t off, len; uint8_t val; char colour, alpha; const char* what; };
const uint64_t kBytes = 256;
const Rule kRules[] = {
    {0, 0, 10, 0, 'C', 'C', "a stream"},
    {0, 8, 9999, 0, 'C', 'A', "colour leaves a coded tile's offset and length to the device; alpha: off & 15"},
    {0, 16, 0, 0, 'C', 'F', "alpha: no stream is empty"},
    {0, 240, 16, 0, 'C', 'C', "a stream that ends the batch: len == bytes - off"},
    {0, 256, 1, 0, 'C', 'A', "alpha: len > bytes - off"},
    {0, 272, 0, 0, 'C', 'A', "alpha: off > bytes"},
    {1, 208, 48, 0, 'R', 'F', "a raw colour tile that ends the batch; alpha: a plane is 16 bytes"},
    {1, 208, 49, 0, 'A', 'A', "one byte past the batch"},
    {1, 240, 16, 0, 'F', 'R', "a raw alpha plane that ends the batch; colour: a raw tile is 48 bytes"},
    {1, 240, 17, 0, 'A', 'A', "one byte past the batch"},
    {1, 0, 47, 0, 'F', 'F', "raw, one byte short"},
    {1, 8, 48, 0, 'A', 'A', "off & 15"},
    {1, 272, 0, 0, 'A', 'A', "off > bytes"},
    {1, 256, 0, 0, 'F', 'F', "off == bytes with len == 0 passes the range; the length is wrong for raw"},
    {2, 256, 0, 77, 'F', 'R', "alpha: a constant at off == bytes with len == 0; colour has no kind 2"},
    {2, 0, 0, 200, 'F', 'R', "alpha: a constant"},
    {2, 0, 1, 9, 'F', 'F', "alpha: a constant with a length"},
    {2, 8, 0, 9, 'F', 'A', "alpha: the range is checked for every kind"},
    {2, 512, 0, 9, 'F', 'A', "alpha: off > bytes"},
    {3, 0, 0, 0, 'F', 'F', "kind 3"},
    {7, 8, 9999, 0, 'F', 'F', "kind 7: the kind is judged before the range"},
};
const uint32_t kNRules = sizeof(kRules) / sizeof(kRules[0]);

int g_fail = 0;
void expect(bool ok, const char* what, uint32_t i) {
  if (!ok) {
    ++g_fail;
    printf("rule failure: %s (entry %u)\n", what, i);
  }
}

bool same_but_windows(const SlotPlan& a, const SlotPlan& b) {
  return a.c_off == b.c_off && a.c_len == b.c_len && a.c_idx == b.c_idx && a.c_pos == b.c_pos && a.s_src == b.s_src &&
         a.s_idx == b.s_idx && a.s_kind == b.s_kind && a.init == b.init && !memcmp(a.by_kind, b.by_kind, sizeof a.by_kind);
}

int rules() {
  // the entries as one row of tiles, all selected
  std::vector<uint64_t> off, len;
  std::vector<uint8_t> kind, val;
  for (const Rule& r : kRules) {
    off.push_back(r.off);
    len.push_back(r.len);
    kind.push_back(r.kind);
    val.push_back(r.val);
  }
  const SlotTables tabs{off.data(), len.data(), kind.data(), val.data(), kBytes};
  const uint32_t first[2] = {0, kNRules}, nx = kNRules, win[5] = {0, 0, 0, 4 * kNRules, 4};
  const SlotWindows g{4, 4, first, &nx, win, 1, true};
  for (int alpha = 0; alpha < 2; ++alpha) {
    SlotPlan p;
    if (alpha) plan_alpha_slots(tabs, g, p); else plan_colour_slots(tabs, g, p);
    expect(p.init.size() == kNRules, "one slot per entry", 0);
    size_t ic = 0, is = 0;
    uint32_t by_kind[3] = {0, 0, 0};
    for (uint32_t i = 0; i < kNRules && p.init.size() == kNRules; ++i) {
      const Rule& r = kRules[i];
      const char want = alpha ? r.alpha : r.colour;
      expect(p.init[i] == (want == 'F' ? NICE_E_FORMAT : want == 'A' ? NICE_E_ARG : NICE_OK), r.what, i);
      if (want == 'F' || want == 'A') continue;
      ++by_kind[r.kind];
      if (want == 'C') {
        expect(ic < p.c_off.size() && p.c_off[ic] == r.off && p.c_len[ic] == r.len && p.c_pos[ic] == i, r.what, i);
        if (!alpha) expect(ic < p.c_idx.size() && p.c_idx[ic] == i && p.c_win[ic] == 0, r.what, i);
      }
      if (alpha || want == 'R') {
        const uint64_t src = !alpha || r.kind == 1 ? r.off : r.kind == 2 ? r.val : ic;
        expect(is < p.s_src.size() && p.s_src[is] == src && p.s_idx[is] == i && p.s_win[is] == 0, r.what, i);
        if (alpha) expect(is < p.s_kind.size() && p.s_kind[is] == r.kind, r.what, i);
        ++is;
      }
      if (want == 'C') ++ic;
    }
    expect(ic == p.c_off.size() && is == p.s_src.size(), "no slot besides the expected ones", 0);
    expect(!memcmp(by_kind, p.by_kind, sizeof by_kind), "counts by kind", 0);
  }
  // the tiled case (no window column) is the one-image, one-window set: the
  // same entries, 21 tiles, as a 7 x 3 grid of a 26 x 11 image, a window over 3 x 3 of them
  const std::vector<uint32_t> w{26}, h{11}, q{0, 5, 3, 10, 6};
  std::vector<uint32_t> sfirst, snx, slot_first(2);
  expect(set_select(w.data(), h.data(), 1, 4, 4, q.data(), 1, sfirst, snx, slot_first.data()) == NICE_OK, "set_select", 0);
  uint32_t tnx, tny;
  TileRange tr;
  expect(tile_select(26, 11, 4, 4, 5, 3, 10, 6, &tnx, &tny, &tr) == NICE_OK, "tile_select", 0);
  expect(tnx * tny == kNRules && sfirst == std::vector<uint32_t>{0, kNRules} && snx == std::vector<uint32_t>{tnx},
         "the grid of the set is the grid of the image", 0);
  expect(tr.tx0 == 1 && tr.ty0 == 0 && tr.tx1 == 4 && tr.ty1 == 3 && slot_first[1] == 9 && tr.count() == 9, "the window's tiles", 0);
  const uint32_t tfirst[2] = {0, tnx * tny};
  for (int alpha = 0; alpha < 2; ++alpha) {
    SlotPlan t, s;
    const SlotWindows gt{4, 4, tfirst, &tnx, q.data(), 1, false}, gs{4, 4, sfirst.data(), snx.data(), q.data(), 1, true};
    if (alpha) { plan_alpha_slots(tabs, gt, t); plan_alpha_slots(tabs, gs, s); }
    else { plan_colour_slots(tabs, gt, t); plan_colour_slots(tabs, gs, s); }
    expect(t.init.size() == 9 && same_but_windows(t, s), "tiled == one-image set, column for column", alpha);
    expect(t.c_win.empty() && t.s_win.empty(), "a tiled plan carries no window column", alpha);
    expect(s.s_win == std::vector<uint32_t>(s.s_src.size(), 0) && (alpha || s.c_win == std::vector<uint32_t>(s.c_off.size(), 0)),
           "the set's window columns are all window 0", alpha);
    expect(table_ok(t, nullptr, 0) && table_ok(s, q.data(), 8), "packer", alpha);
  }
  printf("checked %u entries, %d failures\n", kNRules, g_fail);
  return g_fail ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc == 2 && !strcmp(argv[1], "rules")) return rules();
  fprintf(stderr, "usage: %s sweep | rules\n", argv[0]);
  return 2;
}
