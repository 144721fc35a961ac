"""Image sets, antialiased resized tensor output (include/nice.h, "image sets:
antialiased resized tensor output"), the parts that need no GPU: the tap
ranges, weights, limit and final rounding of csrc/nice_resize.hpp through
tools/resize_arith_check.cpp, against the definition in Python integers and
against the rational triangle; the numpy model that tests/test_sets_resize_aa.py
compares the GPU with, bit for bit; the model's properties and its agreement
with torch's antialiased bilinear; the header, the package and the C++ mirror.

The model: weights by Python integers as the header defines them, h and acc32
in int64 numpy, acc = (acc32 + 128) >> 8, then the element through model_f32 /
bits_of_f32 of tests/test_sets_resize_cpu.py (the single rounding of the exact
rational)."""
import functools
import inspect
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, nice_pkg
from test_sets_tensor_cpu import const_sets, lut32
from test_sets_resize_cpu import (TORCH_SHAPES, bits_of_f32, model_bits, model_f32, positions, random_px, run_tool)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

AA_MAX_IN = 65536


# ---- the definition, in Python integers ---------------------------------------------------
def raw_weights(x, n_in, n_out):
    """(lo, [r_lo .. r_hi]) of output index x of a reducing axis: every i in 0 .. n_in - 1 is looked at."""
    C, S = (2 * x + 1) * n_in, 2 * n_in
    r = [S - abs((2 * i + 1) * n_out - C) for i in range(n_in)]
    taps = [i for i in range(n_in) if r[i] > 0]
    assert taps and taps == list(range(taps[0], taps[-1] + 1))              # one contiguous run, inside the window
    return taps[0], r[taps[0]:taps[-1] + 1]


def weights_of_raw(r):
    R, cum, prev, out = sum(r), 0, 0, []
    for v in r:
        cum += v
        W = (cum * 8192 + R) // (2 * R)
        out.append(W - prev)
        prev = W
    return out


@functools.lru_cache(maxsize=None)
def aa_taps(n_in, n_out, flip=False):
    """Per output index: (lo, (w_lo, ..., w_hi)), weights in 1/4096."""
    out = []
    if n_out >= n_in:
        i0, i1, f = positions(n_in, n_out, flip)
        for a, b, g in zip(i0.tolist(), i1.tolist(), f.tolist()):
            out.append((a, (16 * (256 - g),) + ((16 * g,) if b != a else ())))
        return out
    for x in range(n_out):
        lo, r = raw_weights(n_out - 1 - x if flip else x, n_in, n_out)
        out.append((lo, tuple(weights_of_raw(r))))
    return out


def weight_matrix(n_in, n_out, flip=False):
    m = np.zeros((n_out, n_in), np.int64)
    for x, (lo, w) in enumerate(aa_taps(n_in, n_out, flip)):
        m[x, lo:lo + len(w)] = w
    return m


def model_acc_aa(px, oh, ow, flip=False):
    """[3, oh, ow] int64 accumulators (1/65536) of the uint8 window px [rh, rw, >= 3]."""
    rh, rw = px.shape[:2]
    wx, wy = weight_matrix(rw, ow, flip), weight_matrix(rh, oh)
    b = px[:, :, :3].astype(np.int64).transpose(2, 0, 1)                      # [3, rh, rw]
    h = b @ wx.T                                                             # [3, rh, ow]
    assert h.max() <= 255 << 12
    acc32 = wy[None] @ h                                                     # [3, oh, ow]
    assert acc32.min() >= 0 and acc32.max() <= 255 << 24
    return (acc32 + 128) >> 8


def model_bits_aa(px, oh, ow, flip, scale, bias, dtype):
    """[3, oh, ow] integer bits of the antialiased resized window px."""
    return bits_of_f32(model_f32(model_acc_aa(px, oh, ow, flip), scale, bias), dtype)


def tap_ranges(n_in, n_out, flip=False):
    """(lo, hi) int arrays per output index: the tap rectangle's sides."""
    t = aa_taps(n_in, n_out, flip)
    return np.array([lo for lo, _ in t]), np.array([lo + len(w) - 1 for lo, w in t])


# ---- taps and weights from the tool -------------------------------------------------------
def _parse_aa(lines):
    got = {}
    for line in lines:
        head, _, rest = line.partition(":")
        n_in, n_out, x, lo = (int(v) for v in head.split())
        got.setdefault((n_in, n_out), []).append((lo, tuple(int(v) for v in rest.split())))
    return got


def test_tool_weights_match_the_definition():
    got = _parse_aa(run_tool("aasweep", 40))
    assert len(got) == 1600
    for n_in in range(1, 41):
        for n_out in range(1, 41):
            assert got[n_in, n_out] == aa_taps(n_in, n_out), (n_in, n_out)
    pairs = [(8192, 8191), (2, 1), (3, 2), (515, 9)]
    got = _parse_aa(run_tool("aa", *[v for p in pairs for v in p]))
    for n_in, n_out in pairs:
        assert got[n_in, n_out] == aa_taps(n_in, n_out), (n_in, n_out)


@pytest.mark.parametrize("n_in,n_out", [(65536, 1), (65536, 8192), (65535, 224), (40000, 224)])
def test_tool_weights_of_long_axes(n_in, n_out):
    """Sampled output indices: the range, R, the sum and three weights against the definition."""
    xs = sorted({0, 1 % n_out, n_out // 2, n_out - 1})
    lines = run_tool("aax", n_in, n_out, *xs)
    assert len(lines) == len(xs)
    for x, line in zip(xs, lines):
        gx, lo, hi, R, total, mn, w_lo, w_mid, w_hi = (int(v) for v in line.split())
        want_lo, r = raw_weights(x, n_in, n_out)
        w = weights_of_raw(r)
        assert (gx, lo, hi, R) == (x, want_lo, want_lo + len(r) - 1, sum(r)), x
        assert total == 4096 == sum(w) and mn == min(w) >= 0
        assert (w_lo, w_mid, w_hi) == (w[0], w[(lo + hi) // 2 - lo], w[-1]), x
        assert (2 * x + 1) * n_in < 1 << 32 and (2 * hi + 1) * n_out < 1 << 32 and sum(r) * 8193 < 1 << 64


def test_limit_of_a_reducing_axis():
    assert [int(v) for v in run_tool("aaok", 65537, 8, 65536, 8, 65537, 65537, 1 << 30, 8192, 1 << 30, 8191)] == [0, 1, 1, 0, 0]
    assert [int(v) for v in run_tool("aaround", 0, 127, 128, 383, 384, 255 << 24)] == [0, 0, 1, 1, 2, 255 << 16]


# ---- properties ---------------------------------------------------------------------------
def test_weights_are_the_rational_triangle_to_one_unit():
    for n_in in range(2, 41):
        for n_out in range(1, n_in):
            s = Fraction(n_in, n_out)
            for x, (lo, w) in enumerate(aa_taps(n_in, n_out)):
                c = (x + Fraction(1, 2)) * s
                tri = [max(Fraction(0), 1 - abs(i + Fraction(1, 2) - c) / s) for i in range(n_in)]
                total = sum(tri)
                assert sum(w) == 4096 and min(w) >= 0 and lo >= 0 and lo + len(w) <= n_in
                assert [i for i in range(n_in) if tri[i] > 0] == list(range(lo, lo + len(w)))
                _, r = raw_weights(x, n_in, n_out)
                for k, wk in enumerate(w):
                    assert Fraction(r[k], sum(r)) == tri[lo + k] / total
                    assert abs(Fraction(wk, 4096) - tri[lo + k] / total) < Fraction(1, 4096), (n_in, n_out, x, k)


def test_mirror_non_reducing_and_halving():
    for n_in, n_out in ((13, 5), (30, 1), (40, 39), (5, 13), (7, 7)):
        assert aa_taps(n_in, n_out, True) == aa_taps(n_in, n_out)[::-1]
    for n_in, n_out in ((5, 13), (7, 7), (1, 9)):
        i0, i1, f = positions(n_in, n_out)
        for x, (lo, w) in enumerate(aa_taps(n_in, n_out)):
            assert lo == i0[x] and w == ((16 * (256 - f[x]), 16 * f[x]) if f[x] else (4096,))
            assert lo + len(w) - 1 == i1[x]
    t = aa_taps(14, 7)
    assert all(w == (512, 1536, 1536, 512) for _, w in t[1:-1]) and [lo for lo, _ in t[1:-1]] == [1, 3, 5, 7, 9]
    assert sum(t[0][1]) == 4096 and len(t[0][1]) == 3                       # renormalised at the window's edge


# ---- the model ---------------------------------------------------------------------------------
def test_model_equals_the_plain_model_where_no_axis_reduces():
    nice = nice_pkg()
    scale, bias = const_sets(nice)["imagenet"]
    for k, ((rh, rw), (oh, ow)) in enumerate([((7, 9), (12, 20)), ((3, 3), (32, 32)), ((1, 8), (6, 8)), ((5, 6), (5, 6))]):
        px = random_px(rh, rw, seed=k)
        for flip in (False, True):
            for dtype in ("float32", "bfloat16"):
                assert np.array_equal(model_bits_aa(px, oh, ow, flip, scale, bias, dtype),
                                      model_bits(px, oh, ow, flip, scale, bias, dtype)), ((rh, rw), (oh, ow), flip)


def test_model_identity_is_the_tensor_table_and_white_stays_white():
    nice = nice_pkg()
    px = random_px(13, 9)
    for name, (scale, bias) in const_sets(nice).items():
        table = lut32(scale, bias)
        v = model_f32(model_acc_aa(px, 13, 9), scale, bias)
        assert np.array_equal(v.view(np.int32), np.stack([table[px[:, :, c], c] for c in range(3)]).view(np.int32)), name
    white = np.full((37, 29, 3), 255, np.uint8)
    for size in ((1, 1), (5, 3), (36, 28), (40, 3)):
        assert (model_acc_aa(white, *size) == 255 << 16).all()              # acc32 is 255 * 2^24 exactly, its bound


AA_TORCH_SHAPES = [s for s in TORCH_SHAPES if s[1][1] > 1] + [((29, 37), (6, 8)), ((300, 400), (7, 9)), ((128, 3), (10, 3))]


def axis_bound(n_in, n_out):
    """The largest difference, in grey levels, one axis adds against the exact filter: a reducing axis with at
    most T taps 255 * (T - 1) / 8192 (each cumulative weight is off by at most half of 1/4096, and the sum is
    taken by parts over T - 1 differences of bytes); a non-reducing one 255 / 512 (its position is off by at
    most 1/512 pixel and bilinear interpolation has a slope of at most 255 per pixel)."""
    if n_out >= n_in:
        return 255 / 512
    return 255 * (max(len(w) for _, w in aa_taps(n_in, n_out)) - 1) / 8192


def test_model_agrees_with_torch_antialias():
    """Against interpolate(bilinear, antialias=True) of the crop in float64.  Shapes with ow == 1 are left
    out: there torch itself departs from the triangle; the rational comparison above covers them.  In output
    units: |scale[c]| times the bound plus the two float32 roundings, as tests/test_sets_resize_cpu.py."""
    import torch
    nice = nice_pkg()
    scale, bias = const_sets(nice)["imagenet"]
    worst = 0.0
    assert len(AA_TORCH_SHAPES) == 12
    for k, ((rh, rw), (oh, ow)) in enumerate(AA_TORCH_SHAPES):
        px = random_px(rh, rw, seed=50 + k)
        acc = model_acc_aa(px, oh, ow)
        t = torch.from_numpy(px.astype(np.float64)).permute(2, 0, 1)[None]
        ref = torch.nn.functional.interpolate(t, size=(oh, ow), mode="bilinear", align_corners=False,
                                              antialias=True)[0].numpy()
        bound = axis_bound(rw, ow) + axis_bound(rh, oh) + 2.0 ** -16
        diff = np.abs(acc / 65536.0 - ref).max()
        print((rh, rw), (oh, ow), "difference", diff, "bound", bound)
        worst = max(worst, diff)
        assert diff < bound, ((rh, rw), (oh, ow), diff, bound)
        v = model_f32(acc, scale, bias).astype(np.float64)
        for c in range(3):
            side = (ref[c] * scale[c] + bias[c]).astype(np.float32).astype(np.float64)
            lim = abs(scale[c]) * bound + 2.0 ** -23 * max(np.abs(v[c]).max(), np.abs(side).max())
            assert np.abs(v[c] - side).max() < lim, ((rh, rw), (oh, ow), c)
    print("largest grey-level difference to torch antialias:", worst)


# ---- header, package and mirror ---------------------------------------------------------------
def test_header_package_and_mirror():
    hdr = open(os.path.join(ROOT, "include", "nice.h")).read()
    title = "image sets: antialiased resized tensor output"
    assert title in hdr
    names = set(re.findall(r"\b(nice_[a-z_0-9]+)\s*\(", hdr))
    new = {"nice_set_resize_aa_tensor_dev", "nice_decode_set_resized_aa_dev"}
    assert new <= names
    assert re.search(r"#define\s+NICE_RESIZE_AA_MAX_IN\s+65536u\b", hdr)
    section = hdr[hdr.index(title):hdr.index("one image sharded over ranks")]
    nice = nice_pkg()
    doc = nice.decode_set_resized.__doc__
    for text in ("(cum * 8192 + R) / (2 * R)", "(acc32 + 128) >> 8"):
        assert text in section, text
        assert text in doc, text
    assert "no antialiasing" in doc                                          # the present text stays
    assert new <= set(nice.EXPORTS) and new <= set(nice._signatures())
    assert nice.RESIZE_AA_MAX_IN == AA_MAX_IN
    sig = inspect.signature(nice.decode_set_resized)
    assert "antialias" in sig.parameters and sig.parameters["antialias"].default is False
    assert os.path.exists(os.path.join(ROOT, nice.__name__, "csrc", "nice_sets_resize_aa.hip"))
    assert "nice_decode_set_resized_aa_dev" in open(os.path.join(ROOT, "include", "nice.hpp")).read()
    subprocess.check_call(["make", "-s", "-B", "-C", os.path.join(ROOT, "examples"), "roundtrip"])
