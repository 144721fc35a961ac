"""Image sets on the GPU (include/nice.h, "image sets"): the set split and merge
kernels against numpy on random bytes, the set encode against the oracle tile
by tile and against encode_tiled of every image alone (the defining property),
launch counts that do not depend on the number of images, the decode of images,
windows and crop batches, a damaged tile, the container and the command line.

The helpers are those of tests/test_tiled.py: expected tiles are built in numpy
with the clamp rule, the oracle gives every tile's stream and verdict."""
import ctypes
import dataclasses
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, PKG_NAME
from test_tiled import POISON, crafted_image, device_image, np_tiles, oracle_verdict

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -1, -4
PH_ENC_CLASSIFY, PH_DEC_TABLES, PHASES = 0, 9, 16
CLI = os.path.join(ROOT, PKG_NAME, "cli.py")

# the reference set: (w, h, image source), a SYN-v1 seed or the crafted image whose tile 5 no decoder can read
SIZES = [(200, 136, "crafted"), (333, 211, 3), (65, 1, 4), (5, 7, 6), (64, 64, 7), (130, 70, 9)]
K = len(SIZES)


def _first(shapes, tw, th):
    first = [0]
    for w, h in shapes:
        first.append(first[-1] + (-(-w // tw)) * (-(-h // th)))
    return first


def _touched(w, h, tw, th, x0, y0, rw, rh):
    """The tiles of a rectangle in row-major order (the slots of a window)."""
    nx = -(-w // tw)
    return [ty * nx + tx for ty in range(y0 // th, (y0 + rh - 1) // th + 1)
            for tx in range(x0 // tw, (x0 + rw - 1) // tw + 1)]


class SetRef:
    """The reference set at one channel count and tile size: images, padded
    tiles in global order and the oracle's stream and verdict per tile; built
    once and left unchanged."""

    def __init__(self, O, c, tw, th):
        self.c, self.tw, self.th = c, tw, th
        self.imgs = [crafted_image(O, c) if s == "crafted" else O.gen_syn_v1(w, h, c, s).reshape(h, w, c)
                     for w, h, s in SIZES]
        self.tiles = np.concatenate([np_tiles(im, tw, th) for im in self.imgs])
        self.first = _first([(w, h) for w, h, _ in SIZES], tw, th)
        self.streams, self.kind = [], []
        for t in self.tiles:
            s, k = oracle_verdict(O, t)
            self.streams.append(s)
            self.kind.append(k)


_REFS = {}


def ref(O, c, tw=64, th=64):
    if (c, tw, th) not in _REFS:
        _REFS[c, tw, th] = SetRef(O, c, tw, th)
    return _REFS[c, tw, th]


@pytest.fixture(scope="module")
def ctx(nice):
    return nice.Context(0)


def _cuda(torch, imgs):
    return [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in imgs]


_ENC = {}


def encoded(nice, O, ctx, c, tw=64, th=64):
    """The reference set's ImageSet, encoded once."""
    import torch
    if (c, tw, th) not in _ENC:
        _ENC[c, tw, th] = nice.encode_set(_cuda(torch, ref(O, c, tw, th).imgs), tile=(tw, th), ctx=ctx)
    return _ENC[c, tw, th]


def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _u64s(vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


def _u32s(vals):
    return (ctypes.c_uint32 * len(vals))(*vals)


def test_reference_set_counts(O):
    """The precondition of everything below, from the oracle alone: 46 tiles of
    which exactly global tile 5 (the crafted tile) is outside the format; at
    66 x 70, 37 tiles of which one, in image 1, is."""
    for c in (3, 4):
        r = ref(O, c)
        assert r.first == [0, 12, 36, 38, 39, 40, 46]
        assert r.kind == [1 if t == 5 else 0 for t in range(46)]
    r = ref(O, 3, 66, 70)
    assert r.first == [0, 8, 32, 33, 34, 35, 37]
    raw = [t for t, k in enumerate(r.kind) if k]
    assert len(raw) == 1 and r.first[1] <= raw[0] < r.first[2]


# ---- 1. split and merge alone, on random bytes -------------------------------
def _random_image(w, h, c, seed=0):
    return np.random.default_rng(w * 31 + h * 7 + c + seed).integers(0, 256, (h, w, c), dtype=np.uint8)


# members: (w, h, pitch_extra, base_off)
RGBA_MIX = [(200, 136, 0, 0),     # pitch 800: 16 bytes per lane
            (130, 70, 12, 0),     # row_pitch = 4w + 12: dwords
            (65, 33, 0, 4),       # base 4 bytes past alignment: dwords
            (37, 50, 0, 1),       # base 1 byte past alignment: bytes
            (5, 7, 0, 0), (64, 64, 0, 0)]
SPLIT_CASES = {
    "rgba_mixed_modes": (4, 64, 64, RGBA_MIX),
    "tile_w_66": (4, 66, 70, RGBA_MIX),                                  # no 16-byte path for any member
    "rgb": (3, 64, 64, [(200, 136, 0, 0), (333, 211, 5, 0), (65, 1, 0, 0), (5, 7, 0, 3)]),
    "long_row": (4, 1024, 16, [(700, 40, 0, 0), (9, 20, 0, 4)]),         # a row longer than one unrolled step
}


@pytest.mark.parametrize("name", list(SPLIT_CASES))
def test_split_matches_numpy(nice, ctx, name):
    import torch
    c, tw, th, members = SPLIT_CASES[name]
    imgs = [_random_image(w, h, c, i) for i, (w, h, _, _) in enumerate(members)]
    want = np.concatenate([np_tiles(im, tw, th) for im in imgs])
    n = want.shape[0]
    dev = [device_image(torch, im, pe, bo) for im, (_, _, pe, bo) in zip(imgs, members)]
    before = [raw.clone() for raw, _ in dev]
    args = (_ptrs([v.data_ptr() for _, v in dev]), _u64s([w * c + pe for w, _, pe, _ in members]),
            _u32s([w for w, _, _, _ in members]), _u32s([h for _, h, _, _ in members]), len(members), c, tw, th)
    for stride_extra in (0, 16, 4):
        stride = (tw * th * c + 15) // 16 * 16 + stride_extra
        tiles = torch.full((n * stride + 64,), POISON, dtype=torch.uint8, device="cuda")
        assert nice.lib().nice_set_split_dev(ctx.ptr, None, *args, ctypes.c_void_p(tiles.data_ptr()), stride) == 0
        torch.cuda.synchronize()
        got = tiles.cpu().numpy()
        slots = got[:n * stride].reshape(n, stride)
        assert np.array_equal(slots[:, :tw * th * c].reshape(want.shape), want), stride_extra
        assert (slots[:, tw * th * c:] == POISON).all() and (got[n * stride:] == POISON).all()
    for (raw, _), keep in zip(dev, before):                  # the inputs are only read
        assert torch.equal(raw, keep)


def _merge(nice, ctx, imgs, tw, th, windows, oc, leads, fill=0x7E, failed=(), stray=False):
    """Every (window, tile) slot of `windows` in a shuffled order, merged into
    one poisoned tensor per window whose first pixel is `leads[j]` bytes past a
    16-byte boundary.  `failed`: (window, tile) slots given a nonzero status;
    stray: one more slot whose tile index is outside its image.  Returns what
    each window received and asserts that nothing around it changed."""
    import torch
    c = imgs[0].shape[2]
    tiles = [np_tiles(im, tw, th) for im in imgs]
    slots = [(j, ti) for j, (i, x0, y0, rw, rh) in enumerate(windows)
             for ti in _touched(imgs[i].shape[1], imgs[i].shape[0], tw, th, x0, y0, rw, rh)]
    order = np.random.default_rng(len(slots)).permutation(len(slots))
    slots = [slots[k] for k in order]
    data = [tiles[windows[j][0]][ti].reshape(-1) for j, ti in slots]
    status = [-5 if s in failed else 0 for s in slots]
    if stray:
        j = len(windows) - 1
        slots.append((j, tiles[windows[j][0]].shape[0] + 3))
        data.append(np.full(tw * th * c, 0x11, np.uint8))
        status.append(0)
    ns = len(slots)
    stride = (tw * th * c + 15) // 16 * 16
    buf = torch.full((ns, stride), POISON, dtype=torch.uint8, device="cuda")
    buf[:, :tw * th * c] = torch.from_numpy(np.stack(data)).cuda()
    d_win = torch.tensor([j for j, _ in slots], dtype=torch.int32, device="cuda")
    d_tile = torch.tensor([ti for _, ti in slots], dtype=torch.int32, device="cuda")
    d_st = torch.tensor(status, dtype=torch.int32, device="cuda")
    bigs, ptrs, pitches = [], [], []
    for (i, x0, y0, rw, rh), lead in zip(windows, leads):
        row = (rw * oc + 15) // 16 * 16 + 48
        big = torch.full((rh + 2, row), POISON, dtype=torch.uint8, device="cuda")
        assert big.data_ptr() % 16 == 0
        bigs.append(big)
        ptrs.append(big.data_ptr() + row + 16 + lead)
        pitches.append(row)
    rc = nice.lib().nice_set_merge_dev(
        ctx.ptr, None, ctypes.c_void_p(buf.data_ptr()), stride, None, ctypes.c_void_p(d_win.data_ptr()),
        ctypes.c_void_p(d_tile.data_ptr()), ctypes.c_void_p(d_st.data_ptr()) if failed else None, ns, c,
        _u32s([im.shape[1] for im in imgs]), _u32s([im.shape[0] for im in imgs]), len(imgs), tw, th,
        _u32s([v for wdw in windows for v in wdw]), _ptrs(ptrs), _u64s(pitches), len(windows), oc, fill)
    assert rc == 0
    torch.cuda.synchronize()
    outs = []
    for (i, x0, y0, rw, rh), lead, big in zip(windows, leads, bigs):
        got = big.cpu().numpy()
        outs.append(got[1:1 + rh, 16 + lead:16 + lead + rw * oc].reshape(rh, rw, oc).copy())
        got[1:1 + rh, 16 + lead:16 + lead + rw * oc] = POISON
        assert (got == POISON).all(), (i, x0, y0, rw, rh)
    return outs


def _expect(img, wdw, oc, fill, tw, th, failed_tiles=()):
    """The window's pixels; the parts of `failed_tiles` keep the poison."""
    _, x0, y0, rw, rh = wdw
    c = img.shape[2]
    want = np.full((rh, rw, oc), fill, np.uint8)
    want[:, :, :min(c, oc)] = img[y0:y0 + rh, x0:x0 + rw, :min(c, oc)]
    nx = -(-img.shape[1] // tw)
    for ti in failed_tiles:
        ty, tx = divmod(ti, nx)
        ya, yb = max(ty * th, y0) - y0, min((ty + 1) * th, y0 + rh) - y0
        xa, xb = max(tx * tw, x0) - x0, min((tx + 1) * tw, x0 + rw) - x0
        want[ya:yb, xa:xb] = POISON
    return want


# windows over three images of 200 x 136, 130 x 70 and 37 x 50: whole images,
# regions across tile corners, two windows on one image, x0 % 4 != 0 beside aligned ones
MERGE_SHAPES = [(200, 136), (130, 70), (37, 50)]
MERGE_WINDOWS = [(0, 0, 0, 200, 136), (1, 0, 0, 130, 70), (2, 0, 0, 37, 50),
                 (0, 61, 59, 9, 11), (0, 60, 4, 100, 125),       # across corners, the second 4-pixel aligned
                 (1, 63, 63, 3, 7), (1, 4, 8, 126, 62),
                 (0, 199, 135, 1, 1), (2, 33, 0, 4, 50)]
# first pixel past a 16-byte boundary: 0 (16 bytes per lane where x0 % 4 == 0), 4 (dwords), 1 (bytes)
MERGE_LEADS = [0, 4, 1, 0, 0, 0, 0, 4, 0]


@pytest.mark.parametrize("c,oc,tw,th", [(4, 4, 64, 64), (4, 4, 66, 70), (3, 3, 64, 64), (3, 4, 64, 64), (4, 3, 64, 64)])
def test_merge_matches_numpy(nice, ctx, c, oc, tw, th):
    imgs = [_random_image(w, h, c, i) for i, (w, h) in enumerate(MERGE_SHAPES)]
    outs = _merge(nice, ctx, imgs, tw, th, MERGE_WINDOWS, oc, MERGE_LEADS)
    for wdw, got in zip(MERGE_WINDOWS, outs):
        assert np.array_equal(got, _expect(imgs[wdw[0]], wdw, oc, 0x7E, tw, th)), wdw


def test_merge_long_row(nice, ctx):
    imgs = [_random_image(700, 40, 4), _random_image(9, 20, 4, 1)]
    windows = [(0, 0, 0, 700, 40), (1, 0, 0, 9, 20), (0, 3, 17, 690, 20)]
    outs = _merge(nice, ctx, imgs, 1024, 16, windows, 4, [0, 0, 0])
    for wdw, got in zip(windows, outs):
        assert np.array_equal(got, _expect(imgs[wdw[0]], wdw, 4, 0, 1024, 16)), wdw


def test_merge_skips_failed_and_stray_slots(nice, ctx):
    """A slot with a nonzero status and a tile index outside its image write nothing."""
    imgs = [_random_image(w, h, 4, i) for i, (w, h) in enumerate(MERGE_SHAPES)]
    windows = [(0, 0, 0, 200, 136), (1, 60, 4, 70, 66), (0, 50, 50, 100, 80)]
    failed = {(0, 6), (1, 1), (2, 5)}
    outs = _merge(nice, ctx, imgs, 64, 64, windows, 4, [0, 0, 4], failed=failed, stray=True)
    for j, (wdw, got) in enumerate(zip(windows, outs)):
        lost = [ti for jj, ti in failed if jj == j]
        assert np.array_equal(got, _expect(imgs[wdw[0]], wdw, 4, 0, 64, 64, lost)), wdw


# ---- 2. encode ---------------------------------------------------------------
def _check_encoded(r, iset):
    n = r.first[-1]
    assert iset.first == r.first and iset.widths == [w for w, _, _ in SIZES] and iset.heights == [h for _, h, _ in SIZES]
    assert (iset.channels, iset.tile_w, iset.tile_h) == (r.c, r.tw, r.th)
    lens, off, kind = iset.stream_len.numpy(), iset.off.numpy(), iset.kind.numpy()
    assert off.shape == (n + 1,) and off[0] == 0 and np.array_equal(np.diff(off), (lens + 15) // 16 * 16)
    assert iset.packed.numel() == off[n] == iset.nbytes
    blob = iset.packed.cpu().numpy()
    assert kind.tolist() == r.kind        # 1 exactly where the oracle's tolerant decode raises or differs
    for t in range(n):
        s = blob[off[t]:off[t] + lens[t]].tobytes()
        if kind[t] == 0:
            assert s == r.streams[t], t
        else:
            assert s == r.tiles[t][:, :, :3].tobytes(), t
        assert not blob[off[t] + lens[t]:off[t + 1]].any(), t


@pytest.mark.parametrize("c,tw,th", [(3, 64, 64), (4, 64, 64), (3, 66, 70)])
def test_encode_matches_oracle(nice, O, ctx, c, tw, th):
    _check_encoded(ref(O, c, tw, th), encoded(nice, O, ctx, c, tw, th))


@pytest.mark.parametrize("c", [3, 4])
def test_encode_is_the_concatenation_of_tiled_images(nice, O, ctx, c):
    """The defining property: tile first[i] + t is tile t of encode_tiled of image i alone."""
    import torch
    r = ref(O, c)
    iset = encoded(nice, O, ctx, c)
    blob, off = iset.packed.cpu().numpy(), iset.off.numpy()
    for i, img in enumerate(_cuda(torch, r.imgs)):
        timg = nice.encode_tiled(img, tile=(64, 64), ctx=ctx)
        a, b = r.first[i], r.first[i + 1]
        assert timg.kind.tolist() == iset.kind[a:b].tolist(), i
        assert timg.stream_len.tolist() == iset.stream_len[a:b].tolist(), i
        assert (timg.off + int(off[a])).tolist() == off[a:b + 1].tolist(), i
        assert np.array_equal(timg.packed.cpu().numpy(), blob[off[a]:off[b]]), i


def test_one_image_set_is_the_tiled_image(nice, O, ctx):
    import torch
    img = torch.from_numpy(ref(O, 4).imgs[0]).cuda()
    iset = nice.encode_set([img], tile=(64, 64), ctx=ctx)
    timg = nice.encode_tiled(img, tile=(64, 64), ctx=ctx)
    assert iset.first == [0, 12] and iset.kind.tolist() == [1 if t == 5 else 0 for t in range(12)]
    assert torch.equal(iset.packed, timg.packed) and torch.equal(iset.off, timg.off)
    assert torch.equal(iset.stream_len, timg.stream_len) and torch.equal(iset.kind, timg.kind)


def test_encode_pitched_and_offset_inputs(nice, O, ctx):
    import torch
    r = ref(O, 4)
    layout = [(12, 0), (32, 0), (0, 4), (0, 1), (0, 0), (20, 4)]       # (pitch_extra, base_off) per image
    dev = [device_image(torch, im, pe, bo) for im, (pe, bo) in zip(r.imgs, layout)]
    _check_encoded(r, nice.encode_set([v for _, v in dev], tile=(64, 64), ctx=ctx))
    for (raw, _), (_, bo) in zip(dev, layout):
        assert (raw.view(-1)[:bo] == POISON).all()         # (the inputs are only read)


def test_encode_capacity(nice, O, ctx):
    """Too small a buffer: E_CAPACITY in *d_status, off[n] the size needed, no byte at or past the capacity."""
    import torch
    r = ref(O, 3)
    need = encoded(nice, O, ctx, 3).nbytes
    imgs = _cuda(torch, r.imgs)
    n = r.first[-1]
    buf = torch.full((need + 64,), POISON, dtype=torch.uint8, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    kind = torch.zeros(n, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    rc = nice.lib().nice_encode_set_dev(
        ctx.ptr, None, _ptrs([t.data_ptr() for t in imgs]), _u64s([t.stride(0) if t.shape[0] > 1 else t.shape[1] * 3
                                                                   for t in imgs]),
        _u32s([w for w, _, _ in SIZES]), _u32s([h for _, h, _ in SIZES]), K, 3, 3, 64, 64,
        ctypes.c_void_p(buf.data_ptr()), need - 16, ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(lens.data_ptr()),
        ctypes.c_void_p(kind.data_ptr()), ctypes.c_void_p(status.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    assert int(status[0]) == E_CAPACITY and int(off[n]) == need
    assert bool((buf[need - 16:] == POISON).all())
    with pytest.raises(nice.NiceError) as e:
        nice.encode_set(imgs, tile=(64, 64), ctx=ctx, packed=buf[:need - 16])
    assert e.value.code == E_CAPACITY
    _check_encoded(r, nice.encode_set(imgs, tile=(64, 64), ctx=ctx, packed=buf[:need]))
    assert bool((buf[need:] == POISON).all())
    for bad in ([], [imgs[0], torch.from_numpy(ref(O, 4).imgs[1]).cuda()]):      # K = 0, mixed channels
        with pytest.raises(nice.NiceError) as e:
            nice.encode_set(bad, tile=(64, 64), ctx=ctx)
        assert e.value.code == E_ARG
    with pytest.raises(nice.NiceError) as e:
        nice.encode_set(imgs, tile=(1, 64), ctx=ctx)
    assert e.value.code == E_ARG


# ---- 3. one batch call, whatever the number of images -------------------------
def _timing(nice, ctx):
    L = nice.lib()
    L.nice_ctx_read_timing.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)]
    ms, count = (ctypes.c_double * PHASES)(), (ctypes.c_uint32 * PHASES)()
    assert L.nice_ctx_read_timing(ctx.ptr, ms, count) == 0
    return list(count)


def test_launch_counts_do_not_depend_on_the_number_of_images(nice, O):
    import torch
    ctx = nice.Context(0)
    imgs = _cuda(torch, ref(O, 4).imgs)
    L = nice.lib()
    L.nice_ctx_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.nice_ctx_set_timing(ctx.ptr, 1) == 0
    try:
        one = nice.encode_set(imgs[:1], tile=(64, 64), ctx=ctx)
        enc_one = _timing(nice, ctx)
        six = nice.encode_set(imgs, tile=(64, 64), ctx=ctx)
        enc_six = _timing(nice, ctx)
        assert enc_one[PH_ENC_CLASSIFY] > 0 and enc_one[PH_DEC_TABLES] > 0         # the encode and its verify decode
        assert enc_six[PH_ENC_CLASSIFY] == enc_one[PH_ENC_CLASSIFY]
        assert enc_six[PH_DEC_TABLES] == enc_one[PH_DEC_TABLES]
        nice.decode_set(one, ctx=ctx)
        dec_one = _timing(nice, ctx)
        nice.decode_set(six, ctx=ctx)
        dec_six = _timing(nice, ctx)
        nice.decode_set(six, windows=[(i, 0, 0, 5, 1) for i in range(K)] * 3, ctx=ctx)
        dec_win = _timing(nice, ctx)
        assert dec_one[PH_DEC_TABLES] > 0 and dec_one[PH_ENC_CLASSIFY] == 0
        assert dec_six[PH_DEC_TABLES] == dec_one[PH_DEC_TABLES] == dec_win[PH_DEC_TABLES]
    finally:
        L.nice_ctx_set_timing(ctx.ptr, 0)


# ---- 4. decode ------------------------------------------------------------------
def last_set(nice, ctx):
    L = nice.lib()
    L.nice_test_last_set.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.nice_test_last_set(ctx.ptr, ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value, b.value


@pytest.mark.parametrize("oc", [3, 4])
@pytest.mark.parametrize("c", [3, 4])
def test_decode_all_images(nice, O, ctx, c, oc):
    r = ref(O, c)
    outs = nice.decode_set(encoded(nice, O, ctx, c), out_channels=oc, ctx=ctx)
    assert last_set(nice, ctx) == (45, 1)
    assert len(outs) == K
    for im, out in zip(r.imgs, outs):
        got = out.cpu().numpy()
        assert got.shape == im.shape[:2] + (oc,)
        assert np.array_equal(got[:, :, :3], im[:, :, :3])
        if oc == 4:
            assert (got[:, :, 3] == 255).all()


def test_decode_alpha_without_fill(nice, O, ctx):
    r = ref(O, 3)
    for im, out in zip(r.imgs, nice.decode_set(encoded(nice, O, ctx, 3), out_channels=4, flags=0, ctx=ctx)):
        got = out.cpu().numpy()
        assert np.array_equal(got[:, :, :3], im) and (got[:, :, 3] == 0).all()


def test_decode_subset_into_strided_views(nice, O, ctx):
    import torch
    r = ref(O, 4)
    iset = encoded(nice, O, ctx, 4)
    pick = [4, 1, 3]
    outs = nice.decode_set(iset, images=pick, out_channels=3, ctx=ctx)
    assert last_set(nice, ctx) == (26, 0)
    assert [tuple(o.shape) for o in outs] == [r.imgs[i].shape[:2] + (3,) for i in pick]
    for i, out in zip(pick, outs):
        assert np.array_equal(out.cpu().numpy(), r.imgs[i][:, :, :3])
    bigs = [torch.full((r.imgs[i].shape[0] + 2, r.imgs[i].shape[1] + 5, 4), POISON, dtype=torch.uint8, device="cuda")
            for i in pick]
    views = [b[1:-1, 3:-2] for b in bigs]
    back = nice.decode_set(iset, images=pick, out=views, ctx=ctx)
    assert all(a is b for a, b in zip(back, views))
    for i, big in zip(pick, bigs):
        got = big.cpu().numpy()
        assert np.array_equal(got[1:-1, 3:-2, :3], r.imgs[i][:, :, :3]) and (got[1:-1, 3:-2, 3] == 255).all()
        got[1:-1, 3:-2] = POISON
        assert (got == POISON).all()


# eight windows of 48 x 40 from four images
CROPS = [(0, 70, 70, 48, 40),         # inside the raw tile
         (0, 40, 40, 48, 40),         # across four tiles, the raw one among them
         (0, 152, 96, 48, 40),        # the image's right and bottom edge
         (1, 100, 100, 48, 40), (1, 285, 171, 48, 40),
         (4, 16, 24, 48, 40),
         (5, 82, 30, 48, 40), (5, 0, 0, 48, 40)]


def _slot_counts(r, windows):
    kinds = [r.kind[r.first[i] + ti] for i, x0, y0, rw, rh in windows
             for ti in _touched(SIZES[i][0], SIZES[i][1], r.tw, r.th, x0, y0, rw, rh)]
    return kinds.count(0), kinds.count(1)


@pytest.mark.parametrize("c,oc", [(3, 3), (4, 4), (3, 4)])
def test_crop_batch(nice, O, ctx, c, oc):
    import torch
    r = ref(O, c)
    iset = encoded(nice, O, ctx, c)
    out = torch.full((len(CROPS), 40, 48, oc), POISON, dtype=torch.uint8, device="cuda")
    assert nice.decode_set(iset, windows=CROPS, out=out, ctx=ctx) is out
    assert last_set(nice, ctx) == _slot_counts(r, CROPS) and _slot_counts(r, CROPS)[1] == 2
    got = out.cpu().numpy()
    for j, (i, x0, y0, rw, rh) in enumerate(CROPS):
        assert np.array_equal(got[j, :, :, :3], r.imgs[i][y0:y0 + rh, x0:x0 + rw, :3]), j
    if oc == 4:
        assert (got[:, :, :, 3] == 255).all()
    small = [(3, 1, 2, 3, 4), (2, 60, 0, 5, 1), (3, 0, 0, 5, 7), (2, 0, 0, 65, 1)]
    outs = nice.decode_set(iset, windows=small, out_channels=oc, ctx=ctx)
    assert last_set(nice, ctx) == _slot_counts(r, small) == (6, 0)
    for (i, x0, y0, rw, rh), o in zip(small, outs):
        assert np.array_equal(o.cpu().numpy()[:, :, :3], r.imgs[i][y0:y0 + rh, x0:x0 + rw, :3]), (i, x0, y0)


def test_damaged_tile_fails_alone(nice, O, ctx):
    """Bytes flipped in one coded tile of image 1: its slots fail, in every
    window that touches it, and keep their pixels; everything else is written."""
    import torch
    r = ref(O, 4)
    iset = encoded(nice, O, ctx, 4)
    bad_ti = 7                                             # tile (1, 1) of image 1's 6 x 4 grid
    bad_t = r.first[1] + bad_ti
    assert r.kind[bad_t] == 0
    packed = iset.packed.clone()
    packed[int(iset.off[bad_t]) + 13 + 3] ^= 0xFF          # inside the table header, which follows the 13-byte file header
    hurt = dataclasses.replace(iset, packed=packed)
    outs = [torch.full(im.shape[:2] + (4,), POISON, dtype=torch.uint8, device="cuda") for im in r.imgs]
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set(hurt, out=outs, ctx=ctx)
    st = e.value.statuses
    assert len(st) == 46 and st[bad_t] < 0 and [s for t, s in enumerate(st) if t != bad_t] == [0] * 45
    assert all(a is b for a, b in zip(e.value.out, outs))
    for i, (im, out) in enumerate(zip(r.imgs, outs)):
        want = np.concatenate([im[:, :, :3], np.full(im.shape[:2] + (1,), 255, np.uint8)], axis=2)
        if i == 1:
            want[64:128, 64:128] = POISON                  # the damaged tile's pixels keep the poison
        assert np.array_equal(out.cpu().numpy(), want), i
    # two windows on that tile and one beside it: the tile fails once per window
    windows = [(1, 60, 60, 10, 10), (1, 70, 70, 20, 20), (1, 130, 70, 20, 20)]
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set(hurt, windows=windows, out_channels=3, ctx=ctx)
    st = e.value.statuses
    assert len(st) == 6 and [s < 0 for s in st] == [False, False, False, True, True, False]
    assert np.array_equal(e.value.out[2].cpu().numpy(), r.imgs[1][70:90, 130:150, :3])
    assert np.array_equal(e.value.out[0].cpu().numpy()[:4, :4], r.imgs[1][60:64, 60:64, :3])
    # a raw tile of the wrong length, and a kind that is neither
    lens = iset.stream_len.clone()
    lens[5] -= 1
    kind = iset.kind.clone()
    kind[12] = 2
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set(dataclasses.replace(iset, stream_len=lens, kind=kind),
                        windows=[(0, 64, 64, 10, 10), (1, 0, 0, 65, 10)], ctx=ctx)
    assert e.value.statuses == [nice.E_FORMAT, nice.E_FORMAT, 0]


def test_decode_rejects(nice, O, ctx):
    import torch
    iset = encoded(nice, O, ctx, 3)
    for windows in ([(0, 150, 100, 51, 1)], [(0, 150, 100, 1, 37)], [(3, 0, 0, 6, 1)], [(0, 0, 0, 1, 1), (2, 0, 1, 1, 1)],
                    [(0, 0, 0, 0, 1)], [(K, 0, 0, 1, 1)]):
        with pytest.raises(nice.NiceError) as e:
            nice.decode_set(iset, windows=windows, ctx=ctx)
        assert e.value.code == E_ARG, windows
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set(iset, images=[K], ctx=ctx)
    assert e.value.code == E_ARG
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set(iset, flags=nice.DEC_STRICT_REFERENCE, ctx=ctx)
    assert e.value.code == E_ARG
    two = [(0, 0, 0, 48, 40), (1, 0, 0, 48, 40)]
    for shape in ((2, 48, 40, 3), (3, 40, 48, 3), (2, 40, 48), (2, 40, 48, 5)):
        with pytest.raises(nice.NiceError) as e:
            nice.decode_set(iset, windows=two, out=torch.empty(shape, dtype=torch.uint8, device="cuda"), ctx=ctx)
        assert e.value.code == E_ARG, shape
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set(iset, windows=two, out=[torch.empty((40, 48, 3), dtype=torch.uint8, device="cuda")], ctx=ctx)
    assert e.value.code == E_ARG
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set(iset, images=[0], windows=two, ctx=ctx)
    assert e.value.code == E_ARG


# ---- 5. container and command line -----------------------------------------------
def test_container_round_trip(nice, O, ctx, tmp_path):
    import torch
    r = ref(O, 4)
    iset = encoded(nice, O, ctx, 4)
    path = str(tmp_path / "set.nices")
    nice.save_set(path, iset)
    back = nice.load_set(path, device="cuda")
    assert back.packed.is_cuda and torch.equal(back.packed, iset.packed)
    assert torch.equal(back.off, iset.off) and torch.equal(back.kind, iset.kind) and back.first == iset.first
    for im, out in zip(r.imgs, nice.decode_set(back, out_channels=3, ctx=ctx)):
        assert np.array_equal(out.cpu().numpy(), im[:, :, :3])
    cpu = nice.load_set(path)
    assert not cpu.packed.is_cuda
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set(cpu, ctx=ctx)
    assert e.value.code == E_ARG


def test_cli_directory_set_directory(nice, O, tmp_path):
    """(three small RGBA PNGs: three processes)"""
    png = importlib.import_module(PKG_NAME + ".png")
    r = ref(O, 4)
    pick = [0, 3, 5]
    src = tmp_path / "in"
    src.mkdir()
    for k, i in enumerate(pick):
        h, w, c = r.imgs[i].shape
        png.write_png(str(src / f"img{k}.png"), r.imgs[i].reshape(-1), w, h, c)
    run = subprocess.run([sys.executable, CLI, "--set", str(src), str(tmp_path / "out"), "--tile", "64x64"],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "images: 3 tiles: 19 raw: 1" in run.stdout
    iset = nice.load_set(str(tmp_path / "out.nices"))
    assert (iset.widths, iset.heights, iset.channels) == ([200, 5, 130], [136, 7, 70], 4)
    run = subprocess.run([sys.executable, CLI, str(tmp_path / "out.nices"), str(tmp_path / "back")],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert sorted(os.listdir(tmp_path / "back")) == ["000000.png", "000001.png", "000002.png"]
    for k, i in enumerate(pick):
        got, gw, gh, gc = png.read_png(str(tmp_path / "back" / f"{k:06d}.png"))
        h, w, _ = r.imgs[i].shape
        assert (gw, gh, gc) == (w, h, 3) and np.array_equal(got.reshape(h, w, 3), r.imgs[i][:, :, :3])
    run = subprocess.run([sys.executable, CLI, str(tmp_path / "out.nices"), str(tmp_path / "one.png"), "--index", "2"],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got, gw, gh, gc = png.read_png(str(tmp_path / "one.png"))
    assert (gw, gh, gc) == (130, 70, 3) and np.array_equal(got.reshape(70, 130, 3), r.imgs[5][:, :, :3])


# ---- 6. a realistic size, once ------------------------------------------------------
def test_real_size(nice, O, ctx):
    import torch
    shapes = [(1920, 1080, 2), (1000, 1500, 3), (640, 480, 4)]
    imgs = [O.gen_syn_v1(w, h, 3, s).reshape(h, w, 3) for w, h, s in shapes]
    dev = _cuda(torch, imgs)
    tw, th = nice.DEFAULT_SET_TILE
    iset = nice.encode_set(dev, ctx=ctx)
    assert (iset.tile_w, iset.tile_h) == (tw, th)
    assert iset.first == _first([(w, h) for w, h, _ in shapes], tw, th)
    blob, off = iset.packed.cpu().numpy(), iset.off.numpy()
    for i, img in enumerate(dev):
        timg = nice.encode_tiled(img, tile=(tw, th), ctx=ctx)
        a, b = iset.first[i], iset.first[i + 1]
        assert timg.kind.tolist() == iset.kind[a:b].tolist() and timg.stream_len.tolist() == iset.stream_len[a:b].tolist()
        assert (timg.off + int(off[a])).tolist() == off[a:b + 1].tolist()
        assert np.array_equal(timg.packed.cpu().numpy(), blob[off[a]:off[b]]), i
    for im, out in zip(imgs, nice.decode_set(iset, ctx=ctx)):
        assert np.array_equal(out.cpu().numpy(), im)
    crop = nice.decode_set(iset, windows=[(1, 500, 1000, 224, 224)], ctx=ctx)[0]
    assert np.array_equal(crop.cpu().numpy(), imgs[1][1000:1224, 500:724])
    assert sum(last_set(nice, ctx)) == 4
