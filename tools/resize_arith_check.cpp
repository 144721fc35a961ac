// resize_arith_check -- the arithmetic of the resized tensor output on the CPU:
// the functions of csrc/nice_resize.hpp that the kernel of nice_sets_resize.hip
// runs, and the position-source column of csrc/nice_slot_plan.hpp, printed for
// tests/test_sets_resize_cpu.py to compare with rationals and a plain model.
//   pos N_IN N_OUT [N_IN N_OUT ...]   a line per pair: "n_in n_out: i0,i1,f ..." for x = 0 .. n_out - 1
//   sweep N                            the same for every n_in, n_out in 1 .. N
//   acc B00 B01 B10 B11 FX FY [...]    a line per six numbers: the accumulator
//   unit ACC [...]                     a line per number: the bits of acc / 65536 in binary32, hex
//   aa N_IN N_OUT [N_IN N_OUT ...]   antialiased weights, a line per output index: "n_in n_out x lo: w ..."
//                                      (the taps lo, lo + 1, ...; the two taps of resize_pos where n_out >= n_in)
//   aasweep N                          the same for every n_in, n_out in 1 .. N
//   aax N_IN N_OUT X [X ...]           a line per index: "x lo hi R sum min w_lo w_mid w_hi" (mid = (lo + hi) / 2;
//                                      sum and min over all the taps' weights)
//   aaok N_IN N_OUT [...]              a line per pair: 1 where the antialiased entry points take the axis
//   aaround ACC32 [...]                a line per number: the accumulator in 1/65536
//   src TW TH BYTES K (W H)*K M (I X Y W H)*M (KIND OFF LEN)*n
//                                      a line per slot position: "p kind value init"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../fast-losless-image-compression-format_amd/csrc/nice_resize.hpp"
#include "../fast-losless-image-compression-format_amd/csrc/nice_slot_plan.hpp"

static void print_pos(uint32_t n_in, uint32_t n_out) {
  printf("%u %u:", n_in, n_out);
  for (uint32_t x = 0; x < n_out; ++x) {
    const nice::ResizePos p = nice::resize_pos(x, n_in, n_out);
    printf(" %u,%u,%u", p.i0, p.i1, p.f);
  }
  printf("\n");
}

static void print_aa(uint32_t n_in, uint32_t n_out) {
  for (uint32_t x = 0; x < n_out; ++x) {
    if (n_out >= n_in) {
      const nice::ResizePos p = nice::resize_pos(x, n_in, n_out);
      printf("%u %u %u %u: %u", n_in, n_out, x, p.i0, nice::resize_aa_w0(p.f));
      if (p.i1 != p.i0) printf(" %u", nice::resize_aa_w1(p.f));
    } else {
      const nice::ResizeAaRange r = nice::resize_aa_range(x, n_in, n_out);
      const uint64_t R = nice::resize_aa_cum(r.hi, r.lo, x, n_in, n_out);
      printf("%u %u %u %u:", n_in, n_out, x, r.lo);
      for (uint32_t i = r.lo; i <= r.hi; ++i) printf(" %u", nice::resize_aa_weight(i, r.lo, R, x, n_in, n_out));
    }
    printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::vector<uint64_t> v;
  for (int i = 2; i < argc; ++i) v.push_back(strtoull(argv[i], nullptr, 0));
  const char* mode = argv[1];
  if (!strcmp(mode, "pos") && v.size() % 2 == 0) {
    for (size_t i = 0; i < v.size(); i += 2) print_pos((uint32_t)v[i], (uint32_t)v[i + 1]);
  } else if (!strcmp(mode, "sweep") && v.size() == 1) {
    for (uint32_t n_in = 1; n_in <= v[0]; ++n_in)
      for (uint32_t n_out = 1; n_out <= v[0]; ++n_out) print_pos(n_in, n_out);
  } else if (!strcmp(mode, "acc") && v.size() % 6 == 0) {
    for (size_t i = 0; i < v.size(); i += 6)
      printf("%u\n", nice::resize_acc((uint32_t)v[i], (uint32_t)v[i + 1], (uint32_t)v[i + 2], (uint32_t)v[i + 3],
                                      (uint32_t)v[i + 4], (uint32_t)v[i + 5]));
  } else if (!strcmp(mode, "unit")) {
    for (uint64_t a : v) {
      const float f = nice::resize_unit((uint32_t)a);
      uint32_t bits;
      memcpy(&bits, &f, 4);
      printf("%08x\n", bits);
    }
  } else if (!strcmp(mode, "aa") && v.size() % 2 == 0) {
    for (size_t i = 0; i < v.size(); i += 2) print_aa((uint32_t)v[i], (uint32_t)v[i + 1]);
  } else if (!strcmp(mode, "aasweep") && v.size() == 1) {
    for (uint32_t n_in = 1; n_in <= v[0]; ++n_in)
      for (uint32_t n_out = 1; n_out <= v[0]; ++n_out) print_aa(n_in, n_out);
  } else if (!strcmp(mode, "aax") && v.size() >= 2 && v[1] < v[0]) {
    const uint32_t n_in = (uint32_t)v[0], n_out = (uint32_t)v[1];
    for (size_t k = 2; k < v.size(); ++k) {
      const uint32_t x = (uint32_t)v[k];
      const nice::ResizeAaRange r = nice::resize_aa_range(x, n_in, n_out);
      const uint64_t R = nice::resize_aa_cum(r.hi, r.lo, x, n_in, n_out);
      uint64_t sum = 0;
      uint32_t mn = ~0u;
      for (uint32_t i = r.lo; i <= r.hi; ++i) {
        const uint32_t w = nice::resize_aa_weight(i, r.lo, R, x, n_in, n_out);
        sum += w;
        mn = w < mn ? w : mn;
      }
      printf("%u %u %u %llu %llu %u %u %u %u\n", x, r.lo, r.hi, (unsigned long long)R, (unsigned long long)sum, mn,
             nice::resize_aa_weight(r.lo, r.lo, R, x, n_in, n_out),
             nice::resize_aa_weight((r.lo + r.hi) / 2, r.lo, R, x, n_in, n_out),
             nice::resize_aa_weight(r.hi, r.lo, R, x, n_in, n_out));
    }
  } else if (!strcmp(mode, "aaok") && v.size() % 2 == 0) {
    for (size_t i = 0; i < v.size(); i += 2) printf("%d\n", nice::resize_aa_axis_ok((uint32_t)v[i], (uint32_t)v[i + 1]) ? 1 : 0);
  } else if (!strcmp(mode, "aaround")) {
    for (uint64_t a : v) printf("%u\n", nice::resize_aa_round((uint32_t)a));
  } else if (!strcmp(mode, "src") && v.size() >= 5) {
    size_t at = 0;
    const uint32_t tw = (uint32_t)v[at++], th = (uint32_t)v[at++];
    const uint64_t bytes = v[at++];
    const uint32_t K = (uint32_t)v[at++];
    if (v.size() < at + 2ull * K + 1) return 2;
    std::vector<uint32_t> w(K), h(K);
    for (uint32_t i = 0; i < K; ++i) {
      w[i] = (uint32_t)v[at++];
      h[i] = (uint32_t)v[at++];
    }
    const uint32_t M = (uint32_t)v[at++];
    if (v.size() < at + 5ull * M) return 2;
    std::vector<uint32_t> win(5ull * M);
    for (auto& q : win) q = (uint32_t)v[at++];
    std::vector<uint32_t> first, nx, slot_first((size_t)M + 1);
    if (nice::set_select(w.data(), h.data(), K, tw, th, win.data(), M, first, nx, slot_first.data())) return 3;
    const uint32_t n = first[K];
    if (v.size() != at + 3ull * n) return 2;
    std::vector<uint64_t> off(n), len(n);
    std::vector<uint8_t> kind(n);
    for (uint32_t t = 0; t < n; ++t) {
      kind[t] = (uint8_t)v[at++];
      off[t] = v[at++];
      len[t] = v[at++];
    }
    nice::SlotPlan plan;
    nice::plan_colour_slots(nice::SlotTables{off.data(), len.data(), kind.data(), nullptr, bytes},
                            nice::SlotWindows{tw, th, first.data(), nx.data(), win.data(), M, true}, plan);
    std::vector<uint64_t> src;
    nice::slot_position_sources(plan, src);
    if (src.size() != slot_first[M]) return 3;
    for (size_t p = 0; p < src.size(); ++p)
      printf("%zu %u %llu %d\n", p, (unsigned)(src[p] >> 62), (unsigned long long)(src[p] & nice::SLOT_SRC_VALUE),
             (int)plan.init[p]);
  } else {
    return 2;
  }
  return 0;
}
