"""Image sets, resized tensor output (include/nice.h, "image sets: resized
tensor output"), the parts that need no GPU: the coordinate and accumulator
arithmetic of csrc/nice_resize.hpp and the position column of
csrc/nice_slot_plan.hpp through tools/resize_arith_check.cpp (plain g++, built
by tools/Makefile), against rationals; the numpy reference model that
tests/test_sets_resize.py compares the GPU with, bit for bit; the model's
identity, halving and torch-agreement properties; the header and the package.

The model: positions by Python integers, acc by int64 numpy, then the float32
element as the single rounding of the exact rational acc * scale / 65536 + bias.
acc / 65536 and its product with a float32 scale are exact in double (24 and 48
significant bits); the sum with the bias need not be, so every distinct
(acc, channel) is checked with rationals and, where the double sum is inexact,
rounded from the rational directly."""
import atexit
import functools
import os
import re
import shutil
import struct
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, nice_pkg
from test_sets_tensor_cpu import const_sets, f32, lut32

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

DTYPES = ["float32", "float16", "bfloat16"]


# ---- the tool -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tool():
    d = tempfile.mkdtemp(prefix="resize_arith_check_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools"), os.path.join(d, "resize_arith_check"),
                           "OUT=" + d + os.sep])
    return os.path.join(d, "resize_arith_check")


def run_tool(*args):
    out = subprocess.run([tool()] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.splitlines()


# ---- the model ------------------------------------------------------------------------
def positions(n_in, n_out, flip=False):
    """(i0, i1, f) as int64 arrays of n_out entries: the definition, in Python integers."""
    i0, i1, f = [], [], []
    for x in range(n_out):
        xx = n_out - 1 - x if flip else x
        t = ((2 * xx + 1) * n_in * 256 + n_out) // (2 * n_out)
        q = min(max(t - 128, 0), (n_in - 1) * 256)
        i0.append(q >> 8)
        f.append(q & 255)
        i1.append(min(i0[-1] + (1 if f[-1] else 0), n_in - 1))
    return np.array(i0, np.int64), np.array(i1, np.int64), np.array(f, np.int64)


def model_acc(px, oh, ow, flip=False):
    """[3, oh, ow] int64 accumulators of the uint8 window px [rh, rw, >= 3]."""
    rh, rw = px.shape[:2]
    i0, i1, fx = positions(rw, ow, flip)
    j0, j1, fy = positions(rh, oh)
    b = px[:, :, :3].astype(np.int64)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = (256 - fx) * b[j0][:, i0] + fx * b[j0][:, i1]
    bot = (256 - fx) * b[j1][:, i0] + fx * b[j1][:, i1]
    acc = (256 - fy) * top + fy * bot
    assert acc.min() >= 0 and acc.max() <= 255 * 65536
    return np.ascontiguousarray(acc.transpose(2, 0, 1))


def round_f32(q):
    """The rational q rounded once to float32, to nearest even (normal range only)."""
    if q == 0:
        return 0.0
    sign, q = (-1.0, -q) if q < 0 else (1.0, q)
    e = 0
    while q >= 1 << 24:
        q, e = q / 2, e + 1
    while q < 1 << 23:
        q, e = q * 2, e - 1
    n, rest = divmod(q.numerator, q.denominator)
    twice = 2 * rest
    if twice > q.denominator or (twice == q.denominator and n & 1):
        n += 1
    assert -126 - 23 <= e <= 127 - 23, "outside the normal float32 range"
    return sign * float(n) * 2.0 ** e


_ELEM = {}
_STATS = {"exact": 0, "inexact": 0}


def model_f32(acc, scale, bias):
    """[3, oh, ow] float32: the single rounding of acc * scale[c] / 65536 + bias[c]."""
    out = np.empty(acc.shape, np.float32)
    for c in range(3):
        cache = _ELEM.setdefault((scale[c], bias[c]), {})
        s, t = Fraction(scale[c]), Fraction(bias[c])
        vals, inv = np.unique(acc[c], return_inverse=True)
        ref = np.empty(len(vals), np.float32)
        for k, a in enumerate(vals.tolist()):
            if a not in cache:
                exact = Fraction(a, 65536) * s + t
                dbl = a / 65536 * scale[c] + bias[c]                     # the shortcut, valid where it is exact
                assert Fraction(a / 65536 * scale[c]) == Fraction(a, 65536) * s
                if Fraction(dbl) == exact:
                    cache[a] = f32(dbl)
                    _STATS["exact"] += 1
                else:
                    cache[a] = round_f32(exact)
                    _STATS["inexact"] += 1
            ref[k] = cache[a]
        out[c] = ref[inv].reshape(acc[c].shape)
    mag = np.abs(out.astype(np.float64))
    assert np.isfinite(out).all() and ((mag == 0) | ((mag >= 2.0 ** -14) & (mag < 65504.0))).all()   # normal in all three types
    return out


def bits_of_f32(v, dtype):
    """The stored bits of float32 values as signed integers (int32, or int16 for the 16-bit types)."""
    if dtype == "float32":
        return v.view(np.int32).copy()
    if dtype == "float16":
        return v.astype(np.float16).view(np.int16).copy()                 # numpy rounds to nearest even
    u = v.view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16).view(np.int16)   # bfloat16, nearest even


def model_bits(px, oh, ow, flip, scale, bias, dtype):
    """[3, oh, ow] integer bits of the resized window px."""
    return bits_of_f32(model_f32(model_acc(px, oh, ow, flip), scale, bias), dtype)


def random_px(rh, rw, seed=0, c=3):
    return np.random.default_rng(1000 * rh + rw + seed).integers(0, 256, (rh, rw, c), dtype=np.uint8)


# ---- the coordinates ---------------------------------------------------------------------
LARGE_PAIRS = [(1 << 30, 8192), (1 << 30, 1), (1, 8192), (8192, 8192), ((1 << 30) - 1, 8191), (12345, 224),
               (224, 8191), (65537, 4099), ((1 << 24) + 1, 8192), (40000, 224), (37449, 224), (256, 224), (3, 8192)]


def want_positions(n_in, n_out):
    """From rationals: round half up of (x + 1/2) * n_in / n_out * 256, minus 128, clamped."""
    out = []
    for x in range(n_out):
        v = (Fraction(x) + Fraction(1, 2)) * n_in / n_out * 256
        t = (v + Fraction(1, 2)).__floor__()
        q = min(max(t - 128, 0), (n_in - 1) * 256)
        i0, f = q >> 8, q & 255
        out.append((i0, min(i0 + (1 if f else 0), n_in - 1), f))
    return out


def _parse_pos(lines):
    got = {}
    for line in lines:
        head, _, rest = line.partition(":")
        n_in, n_out = (int(v) for v in head.split())
        got[n_in, n_out] = [tuple(int(v) for v in p.split(",")) for p in rest.split()]
    return got


def test_coordinates_match_rationals():
    got = _parse_pos(run_tool("sweep", 40))
    assert len(got) == 1600
    for n_in in range(1, 41):
        for n_out in range(1, 41):
            assert got[n_in, n_out] == want_positions(n_in, n_out), (n_in, n_out)
    got = _parse_pos(run_tool("pos", *[v for pair in LARGE_PAIRS for v in pair]))
    assert (1 << 30, 8192) in got
    for n_in, n_out in LARGE_PAIRS:
        want = want_positions(n_in, n_out)
        assert got[n_in, n_out] == want, (n_in, n_out)
        i0, i1, f = positions(n_in, n_out)
        assert list(zip(i0.tolist(), i1.tolist(), f.tolist())) == want        # the model's, too
    # the numerator crosses 2^32 inside one axis: both divisions of resize_pos occur
    assert (2 * 0 + 1) * 40000 * 256 + 224 < 1 << 32 < (2 * 223 + 1) * 40000 * 256 + 224


def test_coordinate_properties():
    """f == 0 everywhere at the window's own size; taps stay inside the window; a mirror reverses."""
    for n in (1, 2, 7, 40):
        i0, i1, f = positions(n, n)
        assert (f == 0).all() and (i0 == np.arange(n)).all() and (i1 == i0).all()
    for n_in, n_out in ((5, 13), (13, 5), (1, 9), (30, 1)):
        i0, i1, f = positions(n_in, n_out)
        assert (0 <= i0).all() and (i0 <= i1).all() and (i1 < n_in).all() and ((i1 == i0) | (f != 0)).all()
        r0, r1, rf = positions(n_in, n_out, flip=True)
        assert (r0 == i0[::-1]).all() and (r1 == i1[::-1]).all() and (rf == f[::-1]).all()


# ---- the accumulator ---------------------------------------------------------------------------
def test_accumulator_matches_the_rational_formula():
    rng = np.random.default_rng(7)
    cases = [tuple(int(v) for v in rng.integers(0, 256, 4)) + (fx, fy)
             for fx in (0, 1, 128, 255) for fy in (0, 1, 128, 255) for _ in range(8)]
    cases += [(255, 255, 255, 255, fx, fy) for fx in (0, 1, 128, 255) for fy in (0, 1, 128, 255)]
    got = [int(v) for v in run_tool("acc", *[v for case in cases for v in case])]
    assert len(got) == len(cases)
    for (b00, b01, b10, b11, fx, fy), acc in zip(cases, got):
        wx, wy = Fraction(fx, 256), Fraction(fy, 256)
        exact = (1 - wy) * ((1 - wx) * b00 + wx * b01) + wy * ((1 - wx) * b10 + wx * b11)
        assert Fraction(acc, 65536) == exact, (b00, b01, b10, b11, fx, fy)
        assert acc <= 255 * 65536 < 1 << 24
    # acc / 65536 in binary32 is exact
    bits = run_tool("unit", *got, 255 * 65536, 1, 0)
    for acc, hx in zip(got + [255 * 65536, 1, 0], bits):
        assert Fraction(struct.unpack("<f", struct.pack("<I", int(hx, 16)))[0]) == Fraction(acc, 65536)
    # the model's accumulator is the same function
    px = random_px(2, 2)
    for fx_out, fy_out in ((2, 2), (5, 3), (1, 1)):
        acc = model_acc(px, fy_out, fx_out)
        i0, i1, fx = positions(2, fx_out)
        j0, j1, fy = positions(2, fy_out)
        args = [int(v) for y in range(fy_out) for x in range(fx_out)
                for v in (px[j0[y], i0[x], 1], px[j0[y], i1[x], 1], px[j1[y], i0[x], 1], px[j1[y], i1[x], 1], fx[x], fy[y])]
        assert [int(v) for v in run_tool("acc", *args)] == acc[1].reshape(-1).tolist()


# ---- model properties -----------------------------------------------------------------------
def test_model_float_reference_is_the_single_rounding():
    """round_f32 against struct's rounding of exactly representable doubles, ties included; and
    the model takes both routes (exact double sum, rational) on the imagenet constants."""
    for v in (1.0, -1.0, 0.1, 1 / 3, 1e-3, 65503.9, 2.0 ** -14, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -40):
        assert round_f32(Fraction(v)) == f32(v), v
    assert round_f32(Fraction(1) + Fraction(1, 1 << 24)) == 1.0                          # a tie goes to even
    assert round_f32(Fraction(1) + Fraction(3, 1 << 24)) == 1 + 2.0 ** -22
    nice = nice_pkg()
    scale, bias = const_sets(nice)["imagenet"]
    before = dict(_STATS)
    model_f32(model_acc(random_px(9, 11), 14, 17), scale, bias)
    assert _STATS["exact"] > before["exact"]
    assert _STATS["exact"] + _STATS["inexact"] > 0


def test_model_identity_is_the_tensor_table():
    """n_out == n_in on both axes: acc = b << 16, and the bits are decode_set_tensor's table's."""
    nice = nice_pkg()
    px = random_px(13, 9)
    for flip in (False, True):
        acc = model_acc(px, 13, 9, flip)
        want = px[:, ::-1] if flip else px
        assert np.array_equal(acc, want.transpose(2, 0, 1).astype(np.int64) << 16)
    for name, (scale, bias) in const_sets(nice).items():
        table = lut32(scale, bias)
        v = model_f32(model_acc(px, 13, 9), scale, bias)
        assert np.array_equal(v.view(np.int32), np.stack([table[px[:, :, c], c] for c in range(3)]).view(np.int32)), name


def test_model_halving_is_the_block_mean():
    px = random_px(10, 14)
    acc = model_acc(px, 5, 7)
    s = px.astype(np.int64).reshape(5, 2, 7, 2, 3).sum(axis=(1, 3)).transpose(2, 0, 1)
    assert np.array_equal(acc, s << 14)


TORCH_SHAPES = [((7, 9), (12, 20)), ((30, 40), (24, 24)), ((17, 5), (5, 17)), ((1, 8), (6, 6)), ((8, 1), (3, 9)),
                ((23, 31), (23, 31)), ((40, 30), (20, 15)), ((3, 3), (32, 32)), ((19, 27), (7, 5)), ((2, 2), (1, 1))]


def test_model_agrees_with_torch_bilinear():
    """Against interpolate(bilinear, align_corners=False, antialias=False) of the
    crop in float64 the interpolated byte differs by less than 255/256: each
    axis position is off by at most 1/512 pixel, bilinear interpolation has a
    slope of at most 255 per pixel per axis, and the clamps are the same.  In
    output units: |scale[c]| * 255/256 plus the two float32 roundings (the
    model's and that of the torch side, each at most 2^-24 of the value)."""
    import torch
    nice = nice_pkg()
    scale, bias = const_sets(nice)["imagenet"]
    worst = 0.0
    for k, ((rh, rw), (oh, ow)) in enumerate(TORCH_SHAPES):
        px = random_px(rh, rw, seed=k)
        acc = model_acc(px, oh, ow)
        t = torch.from_numpy(px.astype(np.float64)).permute(2, 0, 1)[None]
        ref = torch.nn.functional.interpolate(t, size=(oh, ow), mode="bilinear", align_corners=False,
                                              antialias=False)[0].numpy()
        diff = np.abs(acc / 65536.0 - ref).max()
        worst = max(worst, diff)
        assert diff < 255 / 256, ((rh, rw), (oh, ow), diff)
        v = model_f32(acc, scale, bias).astype(np.float64)
        for c in range(3):
            side = (ref[c] * scale[c] + bias[c]).astype(np.float32).astype(np.float64)
            bound = abs(scale[c]) * 255 / 256 + 2.0 ** -23 * max(np.abs(v[c]).max(), np.abs(side).max())
            assert np.abs(v[c] - side).max() < bound, ((rh, rw), (oh, ow), c)
    print("largest byte difference to torch:", worst)


# ---- the position column ---------------------------------------------------------------------------
def test_position_sources():
    """A 20 x 10 image in 8 x 6 tiles (3 x 2) with coded, raw and refused tiles, two windows."""
    tw, th, raw_len = 8, 6, 8 * 6 * 3
    #        kind, off, len: tile 2 an unknown kind, tile 4 a raw tile of the wrong length, tile 5 raw at a misaligned offset
    tiles = [(0, 0, 100), (1, 112, raw_len), (2, 0, 0), (0, 256, 100), (1, 400, 100), (1, 561, raw_len)]
    windows = [(0, 0, 0, 20, 10), (0, 9, 5, 3, 2)]          # all six tiles; tiles 1 and 4
    args = [tw, th, 4096, 1, 20, 10, len(windows)] + [v for w in windows for v in w] + [v for t in tiles for v in t]
    got = [tuple(int(v) for v in line.split()) for line in run_tool("src", *args)]
    slots = [0, 1, 2, 3, 4, 5, 1, 4]
    want, coded = [], 0
    for p, t in enumerate(slots):
        kind, off, ln = tiles[t]
        if kind == 0:
            want.append((p, 0, coded, 0))                   # dense: the index among the coded slots
            coded += 1
        elif kind != 1:
            want.append((p, 3, 0, -5))
        elif off % 16:
            want.append((p, 3, 0, -1))
        elif ln != raw_len:
            want.append((p, 3, 0, -5))
        else:
            want.append((p, 1, off, 0))                     # raw: the byte offset in the packed batch
    assert got == want


# ---- header and package ---------------------------------------------------------------------------------
def test_header_declares_the_resize_section():
    hdr = open(os.path.join(ROOT, "include", "nice.h")).read()
    assert "image sets: resized tensor output" in hdr
    names = set(re.findall(r"\b(nice_[a-z_0-9]+)\s*\(", hdr))
    assert {"nice_set_resize_tensor_dev", "nice_decode_set_resized_dev"} <= names
    for k, v in {"NICE_RESIZE_MAX": "8192u", "NICE_SRC_DENSE": "0u", "NICE_SRC_RAW": "1u", "NICE_SRC_NONE": "3u"}.items():
        assert re.search(r"#define\s+%s\s+%s\b" % (k, v), hdr), k
    section = hdr[hdr.index("image sets: resized tensor output"):hdr.index("one image sharded over ranks")]
    for text in ("((2x + 1) * n_in * 256 + n_out) / (2 * n_out)", "(n_in - 1) * 256", "0x1p-16f", "no antialiasing"):
        assert text in section, text
    nice = nice_pkg()
    assert {"nice_set_resize_tensor_dev", "nice_decode_set_resized_dev"} <= set(nice.EXPORTS)
    assert set(nice._signatures()) >= {"nice_set_resize_tensor_dev", "nice_decode_set_resized_dev"}
    assert nice.RESIZE_MAX == 8192 and "decode_set_resized" in nice.__all__
    doc = nice.decode_set_resized.__doc__
    assert "no antialiasing" in doc and "((2x + 1) * n_in * 256 + n_out) // (2 * n_out)" in doc
    for name in ("nice_resize.hpp", "nice_sets_resize.hip"):
        assert os.path.exists(os.path.join(ROOT, nice.__name__, "csrc", name)), name


def test_cpp_mirror_compiles_with_the_resize_call():
    subprocess.check_call(["make", "-s", "-B", "-C", os.path.join(ROOT, "examples"), "roundtrip"])
    assert "decode_set_resized" in open(os.path.join(ROOT, "include", "nice.hpp")).read()
