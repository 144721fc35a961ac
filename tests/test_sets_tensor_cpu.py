"""Image sets, tensor output (include/nice.h, "image sets: tensor output"), the
parts that need no GPU: normalize_affine, the exactness on which the table
reference of tests/test_sets_tensor.py rests, and the header.

The reference of an element is fmaf(b, scale, bias) in float32.  For the four
constant sets below b * scale + bias is exact in double (asserted here with
rationals), so rounding that double once to float32 gives the fused result: a
256 x 3 table per constant set, which the GPU tests look pixels up in.

A float16 element is that float32 rounded again.  `halfway` holds the entries
for which rounding the exact sum once, to float16, gives other bits (HALFWAY):
a kernel that fuses the multiply-add with the conversion fails on them, and on
no entry of the other three sets."""
import os
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np

from conftest import ROOT, nice_pkg

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def f32(v):
    """v rounded once to float32, as a Python float."""
    return struct.unpack("<f", struct.pack("<f", v))[0]


def const_sets(nice):
    """name -> (scale, bias), float32 values as Python floats."""
    return {"unit": ((f32(1 / 255),) * 3, (0.0,) * 3),
            "imagenet": nice.normalize_affine(IMAGENET_MEAN, IMAGENET_STD),
            "odd": (tuple(f32(v) for v in (-0.0123, 3.5, 1 / 3)), tuple(f32(v) for v in (7.25, -100, 1e-3))),
            "halfway": (tuple(float.fromhex(v) for v in ("0x1.4234f8p-8", "0x1.3745d4p-6", "0x1.ea8960p-7")),
                        tuple(float.fromhex(v) for v in ("0x1.eabffep-1", "0x1.31fffcp+1", "0x1.abc95cp-1")))}


# channel -> the bytes of `halfway` whose float16 differs between rounding the exact sum once and rounding it to
# float32 first
HALFWAY = {0: (29, 58, 87, 116, 145, 174, 203), 1: (143, 187, 209, 253), 2: (18, 141, 223)}


def lut32(scale, bias):
    """[256, 3] float32: b * scale[c] + bias[c] in double, rounded once."""
    b = np.arange(256, dtype=np.float64)[:, None]
    return (b * np.array(scale, np.float64)[None, :] + np.array(bias, np.float64)[None, :]).astype(np.float32)


def test_normalize_affine_is_the_rounded_double_expression():
    nice = nice_pkg()
    scale, bias = nice.normalize_affine(IMAGENET_MEAN, IMAGENET_STD)
    assert len(scale) == len(bias) == 3
    for c in range(3):
        assert scale[c] == f32(1.0 / (255.0 * IMAGENET_STD[c])) == float(np.float32(1.0 / (255.0 * IMAGENET_STD[c])))
        assert bias[c] == f32(-IMAGENET_MEAN[c] / IMAGENET_STD[c])
        assert scale[c] == f32(scale[c]) and bias[c] == f32(bias[c])          # float32 holds them exactly
    assert nice.normalize_affine((0, 0, 0), (1, 1, 1)) == ((f32(1 / 255),) * 3, (0.0,) * 3)
    assert "float32 constants" in nice.normalize_affine.__doc__
    for bad in (((0.5, 0.5), (1, 1, 1)), ((0.5,) * 3, (1,) * 4)):
        try:
            nice.normalize_affine(*bad)
        except nice.NiceError as e:
            assert e.code == nice.E_ARG
        else:
            raise AssertionError(bad)


def test_table_reference_is_exact_in_double():
    """For every byte and channel of the four constant sets the double
    b * scale + bias equals the rational one: its one rounding to float32 is
    the fused multiply-add's.  And no entry is subnormal or infinite in float32
    or float16, so no flush-to-zero mode can hide or cause a failure."""
    nice = nice_pkg()
    for name, (scale, bias) in const_sets(nice).items():
        table = lut32(scale, bias)
        for c in range(3):
            assert scale[c] == f32(scale[c]) and bias[c] == f32(bias[c]), (name, c)      # float32 holds the constants
            s, t = Fraction(scale[c]), Fraction(bias[c])
            for b in range(256):
                exact = b * s + t
                dbl = float(b) * scale[c] + bias[c]
                assert Fraction(dbl) == exact, (name, b, c)
                assert float(table[b, c]) == f32(dbl)
        mag = np.abs(table.astype(np.float64))
        assert np.isfinite(table).all() and (mag < 65504.0).all(), name
        assert ((mag == 0) | (mag >= 2.0 ** -14)).all(), name              # normal in float16, hence in float32 and bfloat16
        assert np.isfinite(table.astype(np.float16)).all(), name


def test_float16_rounds_twice_and_only_halfway_shows_it():
    """The float16 element is the float32 table rounded again.  Rounding the
    exact sum (the double table) once to float16 instead, as a multiply-add
    fused with its conversion does, differs at exactly the 14 entries of
    HALFWAY, and at no entry of the other three sets: they cannot tell the two
    apart."""
    nice = nice_pkg()
    for name, (scale, bias) in const_sets(nice).items():
        b = np.arange(256, dtype=np.float64)[:, None]
        exact = b * np.array(scale, np.float64)[None, :] + np.array(bias, np.float64)[None, :]
        twice, once = lut32(scale, bias).astype(np.float16), exact.astype(np.float16)
        differ = {c: tuple(int(v) for v in np.nonzero(twice[:, c] != once[:, c])[0]) for c in range(3)}
        assert differ == (HALFWAY if name == "halfway" else {0: (), 1: (), 2: ()}), name
    assert sum(len(v) for v in HALFWAY.values()) == 14


def test_unfused_form_differs():
    """Why the definition says fmaf: for the imagenet constants the unfused
    float32 product and sum differ from it in 389 of the 768 entries."""
    nice = nice_pkg()
    scale, bias = const_sets(nice)["imagenet"]
    b = np.arange(256, dtype=np.float32)[:, None]
    unfused = (b * np.array(scale, np.float32)[None, :]).astype(np.float32) + np.array(bias, np.float32)[None, :]
    assert int((unfused.astype(np.float32) != lut32(scale, bias)).sum()) == 389


def test_header_declares_the_tensor_section():
    hdr = open(os.path.join(ROOT, "include", "nice.h")).read()
    assert "image sets: tensor output" in hdr
    names = set(re.findall(r"\b(nice_[a-z_0-9]+)\s*\(", hdr))
    assert {"nice_set_merge_tensor_dev", "nice_decode_set_tensor_dev"} <= names
    want = {"NICE_TENSOR_F32": "0u", "NICE_TENSOR_F16": "1u", "NICE_TENSOR_BF16": "2u", "NICE_TENSOR_PLANAR": "0u",
            "NICE_TENSOR_INTERLEAVED": "1u"}
    for k, v in want.items():
        assert re.search(r"#define\s+%s\s+%s\b" % (k, v), hdr), k
    nice = nice_pkg()
    assert {"nice_set_merge_tensor_dev", "nice_decode_set_tensor_dev"} <= set(nice.EXPORTS)
    assert (nice.TENSOR_F32, nice.TENSOR_F16, nice.TENSOR_BF16, nice.TENSOR_PLANAR, nice.TENSOR_INTERLEAVED) == (0, 1, 2, 0, 1)


def test_cpp_mirror_still_compiles():
    """include/nice.hpp with its tensor section against nice.h, by plain g++ (examples/roundtrip.cpp)."""
    subprocess.check_call(["make", "-s", "-B", "-C", os.path.join(ROOT, "examples"), "roundtrip"])
    assert os.path.exists(os.path.join(ROOT, "examples", "roundtrip"))
    assert "decode_set_tensor" in open(os.path.join(ROOT, "include", "nice.hpp")).read()
