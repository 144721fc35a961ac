"""The alpha batch of a tiled image on the GPU (include/nice.h, "tiled images:
alpha"): kinds, values, streams and raw planes against the oracle tile by tile,
round trips of whole images and regions, the alpha pass alone (only byte +3 of
the window changes), errors, the opaque image's launch counts, container and
command line.

Expected values are made here from the oracle alone.  Per padded tile: a
constant plane is kind 2; else the oracle's stream of the triplet image, its
tolerant decode, and the two raw rules (decode fails or differs; stream not
shorter than the plane)."""
import ctypes
import dataclasses
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -1, -4
POISON = 0xA5
CLI = os.path.join(ROOT, PKG_NAME, "cli.py")
PH_ENC_CLASSIFY, PH_DEC_TABLES, PHASES = 0, 9, 16


def np_tiles(img, tw, th):
    """[h, w, c] -> [n, th, tw, c], tile t = ty * nx + tx, padded by the clamp rule."""
    h, w, c = img.shape
    nx, ny = -(-w // tw), -(-h // th)
    ys = np.minimum(np.arange(ny * th), h - 1)
    xs = np.minimum(np.arange(nx * tw), w - 1)
    big = img[ys][:, xs]
    return np.ascontiguousarray(big.reshape(ny, th, nx, tw, c).transpose(0, 2, 1, 3, 4).reshape(nx * ny, th, tw, c))


def _paint(img):
    """Alpha 255, then a soft disc around (96, 24) in x [64, 128) y [0, 48),
    uniform random bytes in x [128, 192) y [0, 48), 0 in x [0, 64) y [48, 96)."""
    h, w, _ = img.shape
    img[:, :, 3] = 255
    y, x = np.mgrid[0:48, 64:128]
    img[0:48, 64:128, 3] = np.clip((20 - np.hypot(x - 96, y - 24)) * 255 / 6, 0, 255).astype(np.uint8)
    img[0:48, 128:192, 3] = np.random.default_rng(11).integers(0, 256, (48, 64), dtype=np.uint8)
    img[48:96, 0:64, 3] = 0
    return img


def image_main(O):
    """200 x 120 RGBA: SYN-v1 colour; alpha as _paint, then 17 in x [64, 128)
    y >= 96 and (x - 192) * 30 for x >= 192."""
    img = _paint(O.gen_syn_v1(200, 120, 4, 3).reshape(120, 200, 4).copy())
    img[96:, 64:128, 3] = 17
    img[:, 192:, 3] = ((np.arange(192, 200) - 192) * 30).astype(np.uint8)
    return img


def image_wide(O):
    """256 x 96 RGBA (rows of 1024 bytes): alpha as _paint, then (x - 224) * 8 for x >= 224."""
    img = _paint(O.gen_syn_v1(256, 96, 4, 4).reshape(96, 256, 4).copy())
    img[:, 224:, 3] = ((np.arange(224, 256) - 224) * 8).astype(np.uint8)
    return img


def triplets(A, tw):
    """Plane [th, tw] -> triplet image [th, aw, 3]."""
    aw = -(-tw // 3)
    return np.ascontiguousarray(A[:, np.minimum(np.arange(3 * aw), tw - 1)].reshape(A.shape[0], aw, 3))


def oracle_alpha_tile(O, A):
    """(kind, value, stored bytes, verify failed) of one padded plane, from the oracle."""
    th, tw = A.shape
    if (A == A[0, 0]).all():
        return 2, int(A[0, 0]), b"", False
    trip = triplets(A, tw)
    aw = trip.shape[1]
    s = O.encode(trip, aw, th, 3)
    try:
        px, _ = O.decode(s, O.DEC_TOLERANT)
        ok = np.array_equal(px.reshape(-1), trip.reshape(-1))
    except O.OracleDecodeError:
        ok = False
    if not ok or len(s) >= tw * th:
        return 1, 0, A.tobytes(), not ok
    return 0, 0, s, False


# name: (image, tile_w, tile_h)
CASES = {
    "main": ("main", 64, 48),     # nx = 4 with an 8-pixel edge column, ny = 3 with a 24-pixel edge row
    "tiny": ("main", 9, 8),       # aw = 3: streams no decoder can read, every non-constant tile raw
    "odd": ("main", 50, 40),      # tile_w % 3 != 0 and % 4 != 0: the clamped last triplet, the byte paths
    "wide": ("wide", 64, 48),     # 16-byte aligned base and pitch
}


class Ref:
    """One case's image and the oracle's verdict per tile; built once and left unchanged."""

    def __init__(self, O, name):
        src, self.tw, self.th = CASES[name]
        self.img = image_main(O) if src == "main" else image_wide(O)
        self.h, self.w, _ = self.img.shape
        self.nx, self.ny = -(-self.w // self.tw), -(-self.h // self.th)
        self.n = self.nx * self.ny
        planes = np_tiles(self.img, self.tw, self.th)[:, :, :, 3]
        verdicts = [oracle_alpha_tile(O, A) for A in planes]
        self.kind = [v[0] for v in verdicts]
        self.value = [v[1] for v in verdicts]
        self.stored = [v[2] for v in verdicts]
        self.verify_failed = sum(v[3] for v in verdicts)

    def count(self, k):
        return self.kind.count(k)


_REFS, _ENC = {}, {}


def ref(O, name):
    if name not in _REFS:
        _REFS[name] = Ref(O, name)
    return _REFS[name]


@pytest.fixture(scope="module")
def ctx(nice):
    return nice.Context(0)


def encoded(nice, O, ctx, name):
    """The case's TiledImage with alpha, encoded once."""
    import torch
    if name not in _ENC:
        r = ref(O, name)
        _ENC[name] = nice.encode_tiled(torch.from_numpy(r.img).cuda(), tile=(r.tw, r.th), ctx=ctx, alpha=True)
    return _ENC[name]


def device_image(torch, img, pitch_extra=0, base_off=0):
    """`img` on the GPU as a row-strided view: rows of w*c + pitch_extra bytes,
    the first pixel base_off bytes past a 256-byte boundary."""
    h, w, c = img.shape
    pitch = w * c + pitch_extra
    raw = torch.full((h * pitch + base_off + 64,), POISON, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 256 == 0
    view = raw[base_off:base_off + h * pitch].view(h, pitch)[:, :w * c].view(h, w, c)
    view.copy_(torch.from_numpy(np.ascontiguousarray(img)).cuda())
    return raw, view


# ---- 1. what the oracle says about the cases ---------------------------------
def test_cases_cover_every_kind(O):
    """From the oracle side alone: all three kinds occur, the tiny tiles are the
    verify-failure path, and the odd tiles code, so no case passes on one kind."""
    r = ref(O, "main")
    assert (r.count(2), r.count(0), r.count(1)) == (7, 4, 1)
    assert sorted({v for k, v in zip(r.kind, r.value) if k == 2}) == [0, 17, 255]
    assert r.kind[1] == 0 and r.kind[2] == 1 and r.verify_failed == 0    # the disc codes, the noise is raw by its size
    assert len(r.stored[2]) == 64 * 48
    t = ref(O, "tiny")
    assert t.n == 345 and t.count(2) == 345 - 112 and t.count(1) == 112 and t.count(0) == 0
    assert t.verify_failed == 98
    o = ref(O, "odd")
    assert (o.count(0), o.count(1), o.count(2)) == (9, 2, 1)
    w = ref(O, "wide")
    assert w.count(0) > 0 and w.count(1) > 0 and w.count(2) > 0


# ---- 1b. the range pass alone, on random bytes ------------------------------------
# (w, h, tile_w, tile_h, pitch_extra, base_off): 16 bytes per lane, dwords, bytes; tile origins off the 16-byte
# groups; a row longer than one unrolled step; an image smaller than one tile
RANGE_CASES = [(200, 136, 64, 64, 0, 0), (200, 136, 64, 64, 12, 0), (200, 136, 64, 64, 0, 4), (200, 136, 64, 64, 0, 1),
               (333, 211, 66, 70, 4, 0), (1500, 9, 1300, 8, 0, 0), (5, 7, 64, 64, 12, 0), (65, 1, 64, 64, 0, 0)]


@pytest.mark.parametrize("w,h,tw,th,pitch_extra,base_off", RANGE_CASES)
def test_range_matches_numpy(nice, ctx, w, h, tw, th, pitch_extra, base_off):
    import torch
    rng = np.random.default_rng(w + 3 * h + tw)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    # narrow per-tile ranges, so that a pixel read from a neighbouring tile shows
    lab = (np.arange(h)[:, None] // th) * (-(-w // tw)) + np.arange(w)[None, :] // tw
    img[:, :, 3] = (lab * 37 % 200 + rng.integers(0, 9, (h, w))).astype(np.uint8)
    planes = np_tiles(img, tw, th)[:, :, :, 3].reshape(-1, tw * th)
    _, view = device_image(torch, img, pitch_extra, base_off)
    n = planes.shape[0]
    lo = torch.full((n + 1,), 77, dtype=torch.int32, device="cuda")
    hi = torch.full((n + 1,), 77, dtype=torch.int32, device="cuda")
    rc = nice.lib().nice_tiles_alpha_range_dev(ctx.ptr, None, ctypes.c_void_p(view.data_ptr()), w * 4 + pitch_extra, w, h,
                                               tw, th, ctypes.c_void_p(lo.data_ptr()), ctypes.c_void_p(hi.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    assert lo.cpu().tolist() == planes.min(axis=1).tolist() + [77]
    assert hi.cpu().tolist() == planes.max(axis=1).tolist() + [77]


# ---- 2. encode -----------------------------------------------------------------
def _check_alpha(r, timg):
    a = timg.alpha
    n = r.n
    assert a is not None and (timg.nx, timg.ny) == (r.nx, r.ny)
    lens, off, kind, val = a.stream_len.numpy(), a.off.numpy(), a.kind.numpy(), a.value.numpy()
    assert kind.tolist() == r.kind
    assert val.tolist() == r.value
    assert off.shape == (n + 1,) and off[0] == 0 and np.array_equal(np.diff(off), (lens + 15) // 16 * 16)
    assert a.packed.numel() == off[n] == a.nbytes
    blob = a.packed.cpu().numpy()
    for t in range(n):
        assert blob[off[t]:off[t] + lens[t]].tobytes() == r.stored[t], (t, kind[t])
        assert not blob[off[t] + lens[t]:off[t + 1]].any(), t


@pytest.mark.parametrize("name", list(CASES))
def test_encode_matches_oracle(nice, O, ctx, name):
    r = ref(O, name)
    timg = encoded(nice, O, ctx, name)
    _check_alpha(r, timg)
    assert timg.alpha.packed.is_cuda and not timg.alpha.off.is_cuda


@pytest.mark.parametrize("pitch_extra,base_off", [(12, 0), (0, 4), (0, 1), (32, 0)])
def test_encode_pitched_input(nice, O, ctx, pitch_extra, base_off):
    """The range pass's dword and byte fallbacks (and a pitched 16-byte case)."""
    import torch
    r = ref(O, "wide")
    raw, view = device_image(torch, r.img, pitch_extra, base_off)
    _check_alpha(r, nice.encode_tiled(view, tile=(r.tw, r.th), ctx=ctx, alpha=True))
    assert (raw.view(-1)[:base_off] == POISON).all()


def test_colour_batch_is_untouched(nice, O, ctx):
    """alpha=True changes nothing in the colour batch; the default has no alpha."""
    import torch
    r = ref(O, "main")
    plain = nice.encode_tiled(torch.from_numpy(r.img).cuda(), tile=(r.tw, r.th), ctx=ctx)
    assert plain.alpha is None
    both = encoded(nice, O, ctx, "main")
    assert torch.equal(plain.packed, both.packed) and torch.equal(plain.off, both.off)
    assert torch.equal(plain.stream_len, both.stream_len) and torch.equal(plain.kind, both.kind)
    out = nice.decode_tiled(plain, ctx=ctx).cpu().numpy()           # decodes as before: RGB and the fill
    assert np.array_equal(out[:, :, :3], r.img[:, :, :3]) and (out[:, :, 3] == 255).all()


# ---- 3. decode: whole images and regions -----------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_round_trip(nice, O, ctx, name):
    r = ref(O, name)
    timg = encoded(nice, O, ctx, name)
    out = nice.decode_tiled(timg, ctx=ctx)
    assert tuple(out.shape) == (r.h, r.w, 4)
    assert np.array_equal(out.cpu().numpy(), r.img)
    assert np.array_equal(nice.decode_tiled(timg, flags=0, ctx=ctx).cpu().numpy(), r.img)   # the fill flag is irrelevant
    rgb = nice.decode_tiled(timg, out_channels=3, ctx=ctx)
    assert np.array_equal(rgb.cpu().numpy(), r.img[:, :, :3])


# x0 % 4 != 0 and == 0, across tile edges, inside one constant tile (0, 0), inside the raw tile, the last pixel
ROIS = [(61, 43, 9, 11), (60, 40, 80, 30), (64, 0, 64, 48), (4, 4, 40, 30), (3, 5, 41, 31), (130, 2, 50, 40),
        (8, 0, 192, 120), (199, 119, 1, 1)]


@pytest.mark.parametrize("name", ["main", "odd", "wide"])
def test_decode_region(nice, O, ctx, name):
    import torch
    r = ref(O, name)
    timg = encoded(nice, O, ctx, name)
    for roi in ROIS:
        x0, y0, rw, rh = roi
        if x0 + rw > r.w or y0 + rh > r.h:      # (the last two are the 200 x 120 image's)
            continue
        want = r.img[y0:y0 + rh, x0:x0 + rw]
        assert np.array_equal(nice.decode_tiled(timg, roi=roi, ctx=ctx).cpu().numpy(), want), roi
        # a row-strided out inside a poisoned larger tensor
        big = torch.full((rh + 2, rw + 5, 4), POISON, dtype=torch.uint8, device="cuda")
        win = big[1:1 + rh, 3:3 + rw]
        assert nice.decode_tiled(timg, roi=roi, out=win, ctx=ctx) is win
        got = big.cpu().numpy()
        assert np.array_equal(got[1:1 + rh, 3:3 + rw], want), roi
        got[1:1 + rh, 3:3 + rw] = POISON
        assert (got == POISON).all(), roi


def _alpha_alone(nice, ctx, timg, roi, win, pitch):
    """nice_decode_tiled_alpha_dev alone on the window; the statuses."""
    import torch
    a = timg.alpha
    n = timg.nx * timg.ny
    x0, y0, rw, rh = roi
    tx0, ty0, tx1, ty1 = nice.tile_select(timg.width, timg.height, timg.tile_w, timg.tile_h, *roi)
    m = (tx1 - tx0) * (ty1 - ty0)
    status = torch.full((m,), 99, dtype=torch.int32, device="cuda")
    tabs = [a.off.contiguous(), a.stream_len.contiguous(), a.kind.contiguous(), a.value.contiguous()]
    rc = nice.lib().nice_decode_tiled_alpha_dev(
        ctx.ptr, None, ctypes.c_void_p(a.packed.data_ptr() if a.packed.numel() else None), int(a.off[n]),
        *[ctypes.c_void_p(t.data_ptr()) for t in tabs], timg.width, timg.height, timg.tile_w, timg.tile_h,
        x0, y0, rw, rh, ctypes.c_void_p(win.data_ptr()), pitch, ctypes.c_void_p(status.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    return status.cpu().tolist()


def _pattern(shape):
    return (np.arange(int(np.prod(shape)), dtype=np.int64) * 7 % 251).astype(np.uint8).reshape(shape)


# (lead bytes, pitch slack): window rows 16-byte aligned or not
@pytest.mark.parametrize("lead,slack", [(16, 0), (20, 0), (16, 4), (17, 3)])
@pytest.mark.parametrize("name", ["main", "odd", "wide"])
def test_alpha_pass_writes_only_alpha(nice, O, ctx, name, lead, slack):
    """The alpha call alone on a patterned tensor: byte +3 of the window's
    pixels becomes the image's alpha; the window's colour bytes and every byte
    around the window stay."""
    import torch
    r = ref(O, name)
    timg = encoded(nice, O, ctx, name)
    for roi in [(0, 0, r.w, r.h), (60, 40, 80, 30), (61, 43, 9, 11), (4, 4, 40, 30)]:
        x0, y0, rw, rh = roi
        pitch = (rw * 4 + 15) // 16 * 16 + 32 + slack
        before = _pattern((rh + 2, pitch))
        big = torch.from_numpy(before).cuda()
        assert big.data_ptr() % 256 == 0
        win = big[1:1 + rh, lead:lead + rw * 4]
        st = _alpha_alone(nice, ctx, timg, roi, win, pitch)
        assert st == [0] * len(st)
        want = before.copy()
        want[1:1 + rh, lead:lead + rw * 4].reshape(rh, rw, 4)[:, :, 3] = r.img[y0:y0 + rh, x0:x0 + rw, 3]
        assert np.array_equal(big.cpu().numpy(), want), (roi, lead, slack)


# ---- 4. errors -----------------------------------------------------------------
def test_rgb_image_is_refused(nice, O, ctx):
    import torch
    img = torch.from_numpy(np.ascontiguousarray(ref(O, "main").img[:, :, :3])).cuda()
    with pytest.raises(nice.NiceError) as e:
        nice.encode_tiled(img, tile=(64, 48), ctx=ctx, alpha=True)
    assert e.value.code == E_ARG


def test_encode_capacity(nice, O, ctx):
    """Too small a buffer: NICE_E_CAPACITY, aoff[n] the size needed, nothing at or past the capacity written."""
    import torch
    r = ref(O, "main")
    need = encoded(nice, O, ctx, "main").alpha.nbytes
    px = torch.from_numpy(r.img).cuda()
    n = r.n
    for cap, want in ((need - 16, E_CAPACITY), (need, 0)):
        buf = torch.full((need + 64,), POISON, dtype=torch.uint8, device="cuda")
        off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        lens = torch.zeros(n, dtype=torch.int64, device="cuda")
        kind = torch.zeros(n, dtype=torch.uint8, device="cuda")
        val = torch.zeros(n, dtype=torch.uint8, device="cuda")
        status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        rc = nice.lib().nice_encode_tiled_alpha_dev(
            ctx.ptr, None, ctypes.c_void_p(px.data_ptr()), r.w * 4, r.w, r.h, r.tw, r.th,
            ctypes.c_void_p(buf.data_ptr()), cap, *[ctypes.c_void_p(t.data_ptr()) for t in (off, lens, kind, val, status)])
        assert rc == 0
        torch.cuda.synchronize()
        assert int(status.cpu()[0]) == want
        assert int(off.cpu()[n]) == need
        assert bool((buf[cap:] == POISON).all())
        assert kind.cpu().tolist() == r.kind
    assert nice.tiled_alpha_bound(r.w, r.h, r.tw, r.th) == n * ((max(nice.encode_bound(22, 48), 64 * 48) + 15) // 16 * 16)
    assert nice.tiled_alpha_bound(r.w, r.h, 1, 48) == 0 and nice.lib().nice_tile_alpha_width(50) == 17


def test_damaged_alpha_tile_fails_alone(nice, O, ctx):
    import torch
    r = ref(O, "main")
    timg = encoded(nice, O, ctx, "main")
    a = timg.alpha
    bad_t = 1                                                 # the disc, a coded tile
    packed = a.packed.clone()
    packed[int(a.off[bad_t]) + 7] ^= 0xFF                     # the header's width
    hurt = dataclasses.replace(timg, alpha=dataclasses.replace(a, packed=packed))
    # the alpha call alone: the tile keeps the caller's alpha bytes, the others are written
    before = _pattern((r.h, r.w * 4))
    out = torch.from_numpy(before).cuda()
    st = _alpha_alone(nice, ctx, hurt, (0, 0, r.w, r.h), out, r.w * 4)
    assert len(st) == 12 and st[bad_t] < 0 and [s for t, s in enumerate(st) if t != bad_t] == [0] * 11
    want = before.copy().reshape(r.h, r.w, 4)
    keep = want[0:48, 64:128, 3].copy()
    want[:, :, 3] = r.img[:, :, 3]
    want[0:48, 64:128, 3] = keep
    assert np.array_equal(out.cpu().numpy().reshape(r.h, r.w, 4), want)
    # decode_tiled: both passes' statuses in the error
    with pytest.raises(nice.NiceError) as e:
        nice.decode_tiled(hurt, ctx=ctx)
    assert e.value.statuses == [0] * 12 and e.value.alpha_statuses == st
    got = e.value.out.cpu().numpy()
    want = r.img.copy()
    want[0:48, 64:128, 3] = 255                               # what the colour pass wrote there
    assert np.array_equal(got, want)
    # tables: a kind above 2, a raw length, a constant with a length, an offset off 16
    kind = a.kind.clone()
    kind[0] = 3
    lens = a.stream_len.clone()
    lens[2] -= 1
    lens[4] = 16
    off = a.off.clone()
    off[5] += 8
    broken = dataclasses.replace(timg, alpha=dataclasses.replace(a, kind=kind, stream_len=lens, off=off))
    with pytest.raises(nice.NiceError) as e:
        nice.decode_tiled(broken, roi=(0, 0, 200, 96), ctx=ctx)
    assert e.value.alpha_statuses == [nice.E_FORMAT, 0, nice.E_FORMAT, 0, nice.E_FORMAT, nice.E_ARG, 0, 0]
    assert e.value.statuses == [0] * 8


def test_nothing_left_to_decode(nice, O, ctx):
    """Every tile's kind outside the format, in both batches (100 x 70 at
    64 x 48, 4 tiles): both passes refuse every slot on the host, nothing is
    uploaded or decoded, the output keeps its poison, the counters are zero,
    and the context then decodes the sound image exactly."""
    import torch
    from test_tiled import last_tiled
    w, h, tw, th, n = 100, 70, 64, 48, 4
    img = np.random.default_rng(5).integers(0, 256, (h, w, 4), dtype=np.uint8)
    timg = nice.encode_tiled(torch.from_numpy(img).cuda(), tile=(tw, th), ctx=ctx, alpha=True)
    assert timg.kind.numel() == n
    hurt = dataclasses.replace(timg, kind=torch.full((n,), 7, dtype=torch.uint8),
                               alpha=dataclasses.replace(timg.alpha, kind=torch.full((n,), 3, dtype=torch.uint8)))
    for roi, m in ((None, 4), ((60, 40, 30, 20), 4), ((70, 50, 20, 10), 1)):
        rh, rw = (h, w) if roi is None else (roi[3], roi[2])
        out = torch.full((rh, rw, 4), POISON, dtype=torch.uint8, device="cuda")
        nice.decode_tiled(timg, roi=(0, 0, 1, 1), ctx=ctx)        # (the counters start from a sound decode's)
        assert sum(last_tiled(nice, ctx)) == 1
        with pytest.raises(nice.NiceError) as e:
            nice.decode_tiled(hurt, roi=roi, out=out, ctx=ctx)
        assert e.value.statuses == [nice.E_FORMAT] * m and e.value.alpha_statuses == [nice.E_FORMAT] * m
        assert bool((out == POISON).all())
        assert last_tiled(nice, ctx) == (0, 0)
    assert np.array_equal(nice.decode_tiled(timg, ctx=ctx).cpu().numpy(), img)
    assert sum(last_tiled(nice, ctx)) == n


# ---- 5. the opaque image -----------------------------------------------------------
def _timing(nice, ctx):
    L = nice.lib()
    L.nice_ctx_read_timing.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)]
    ms, count = (ctypes.c_double * PHASES)(), (ctypes.c_uint32 * PHASES)()
    assert L.nice_ctx_read_timing(ctx.ptr, ms, count) == 0
    return list(count)


def test_opaque_image_costs_the_range_pass_only(nice, O):
    import torch
    ctx = nice.Context(0)
    img = O.gen_syn_v1(200, 120, 4, 3).reshape(120, 200, 4).copy()
    img[:, :, 3] = 255
    px = torch.from_numpy(img).cuda()
    L = nice.lib()
    L.nice_ctx_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.nice_ctx_set_timing(ctx.ptr, 1) == 0
    try:
        plain = nice.encode_tiled(px, tile=(64, 48), ctx=ctx)
        enc_plain = _timing(nice, ctx)
        timg = nice.encode_tiled(px, tile=(64, 48), ctx=ctx, alpha=True)
        enc_alpha = _timing(nice, ctx)
        a = timg.alpha
        assert a.kind.tolist() == [2] * 12 and a.value.tolist() == [255] * 12
        assert a.packed.numel() == 0 and a.off.tolist() == [0] * 13 and a.stream_len.tolist() == [0] * 12
        assert enc_plain[PH_ENC_CLASSIFY] > 0 and enc_alpha == enc_plain      # no encode, no decode for the alpha
        out_plain = nice.decode_tiled(plain, ctx=ctx)
        dec_plain = _timing(nice, ctx)
        out = nice.decode_tiled(timg, flags=0, ctx=ctx)
        dec_alpha = _timing(nice, ctx)
        assert dec_plain[PH_DEC_TABLES] > 0 and dec_alpha == dec_plain
        assert np.array_equal(out.cpu().numpy(), img) and torch.equal(out, out_plain)
    finally:
        L.nice_ctx_set_timing(ctx.ptr, 0)


# ---- 6. container and command line -------------------------------------------------
def test_container_round_trip(nice, O, ctx, tmp_path):
    import torch
    r = ref(O, "main")
    timg = encoded(nice, O, ctx, "main")
    path = str(tmp_path / "img.nicet")
    nice.save_tiled(path, timg)
    back = nice.load_tiled(path, device="cuda")
    assert back.alpha.packed.is_cuda and torch.equal(back.alpha.packed, timg.alpha.packed)
    assert torch.equal(back.alpha.kind, timg.alpha.kind) and torch.equal(back.alpha.value, timg.alpha.value)
    assert np.array_equal(nice.decode_tiled(back, ctx=ctx).cpu().numpy(), r.img)
    plain = dataclasses.replace(timg, alpha=None)              # a version 1 file decodes to the same RGB as before
    nice.save_tiled(path, plain)
    v1 = nice.load_tiled(path, device="cuda")
    assert v1.alpha is None
    assert torch.equal(nice.decode_tiled(v1, ctx=ctx), nice.decode_tiled(plain, ctx=ctx))


def test_cli_png_nicet_png(nice, O, tmp_path):
    """(RGBA PNG -> --tile 64x48 --alpha -> .nicet -> RGBA PNG, and a region)"""
    png = importlib.import_module(PKG_NAME + ".png")
    r = ref(O, "main")
    src = str(tmp_path / "in.png")
    png.write_png(src, r.img.reshape(-1), r.w, r.h, 4)
    run = subprocess.run([sys.executable, CLI, src, str(tmp_path / "out"), "--tile", "64x48", "--alpha"],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "tiles: 4x3 raw:" in run.stdout and "alpha tiles: coded: 4 raw: 1 constant: 7" in run.stdout
    assert nice.load_tiled(str(tmp_path / "out.nicet")).alpha.kind.tolist() == r.kind
    run = subprocess.run([sys.executable, CLI, str(tmp_path / "out.nicet"), str(tmp_path / "part.png"), "--roi",
                          "61,43,70,11"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got, gw, gh, gc = png.read_png(str(tmp_path / "part.png"))
    assert (gw, gh, gc) == (70, 11, 4) and np.array_equal(got.reshape(11, 70, 4), r.img[43:54, 61:131])
    run = subprocess.run([sys.executable, CLI, str(tmp_path / "out.nicet"), str(tmp_path / "back")],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got, gw, gh, gc = png.read_png(str(tmp_path / "back.png"))
    assert (gw, gh, gc) == (r.w, r.h, 4) and np.array_equal(got.reshape(r.h, r.w, 4), r.img)
