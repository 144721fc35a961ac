"""The alpha batch of an image set on the GPU (include/nice.h, "image sets:
alpha"): the set range pass against numpy, the encode against the oracle tile
by tile and against encode_tiled(alpha=True) of every image alone (the defining
property), round trips of images, windows and crop batches, the alpha pass
alone (only byte +3 of the windows changes), selection, launch counts that
depend on neither the number of images nor of windows, the opaque set, errors,
the container and the command line.

The helpers are those of tests/test_tiled_alpha.py and tests/test_sets.py.
Expected values are made here from the oracle and numpy alone: per padded tile
of every image a constant plane is kind 2; else the oracle's stream of the
triplet image, its tolerant decode, and the two raw rules."""
import ctypes
import dataclasses
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, PKG_NAME
from test_sets import _cuda, _first, _ptrs, _timing, _touched, _u32s, _u64s
from test_tiled_alpha import POISON, _pattern, device_image, image_main, image_wide, np_tiles, oracle_alpha_tile

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY, E_FORMAT = -1, -4, -5
PH_ENC_CLASSIFY, PH_DEC_TABLES = 0, 9
CLI = os.path.join(ROOT, PKG_NAME, "cli.py")

TILES = [(64, 48), (50, 40), (9, 8)]
K = 6


def ref_images(O):
    """The reference set: six RGBA images whose alpha planes give all three
    kinds, in different images."""
    def syn(w, h, seed):
        return O.gen_syn_v1(w, h, 4, seed).reshape(h, w, 4).copy()
    imgs = [image_main(O), image_wide(O), syn(65, 1, 4), syn(5, 7, 6), syn(130, 70, 9), syn(64, 48, 7)]
    imgs[2][:, :, 3] = 255
    imgs[3][:, :, 3] = np.random.default_rng(5).integers(0, 256, (7, 5)).astype(np.uint8)
    imgs[4][:, :, 3] = (np.arange(130) * 255 // 129).astype(np.uint8)[None, :]
    imgs[5][:, :, 3] = 0
    return imgs


class SetAlphaRef:
    """The reference set at one tile size: the images, `first`, and the
    oracle's verdict per global tile; built once and left unchanged."""

    def __init__(self, O, tw, th):
        self.tw, self.th = tw, th
        self.imgs = ref_images(O)
        self.shapes = [(im.shape[1], im.shape[0]) for im in self.imgs]
        self.first = _first(self.shapes, tw, th)
        self.n = self.first[-1]
        planes = np.concatenate([np_tiles(im, tw, th)[:, :, :, 3] for im in self.imgs])
        verdicts = [oracle_alpha_tile(O, A) for A in planes]
        self.kind = [v[0] for v in verdicts]
        self.value = [v[1] for v in verdicts]
        self.stored = [v[2] for v in verdicts]
        self.verify_failed = sum(v[3] for v in verdicts)

    def count(self, k):
        return self.kind.count(k)

    def slot_kinds(self, windows):
        """The kinds of the windows' slots, in set_select's order."""
        return [self.kind[self.first[i] + ti] for i, x0, y0, rw, rh in windows
                for ti in _touched(*self.shapes[i], self.tw, self.th, x0, y0, rw, rh)]


_REFS, _ENC = {}, {}


def ref(O, tw=64, th=48):
    if (tw, th) not in _REFS:
        _REFS[tw, th] = SetAlphaRef(O, tw, th)
    return _REFS[tw, th]


@pytest.fixture(scope="module")
def ctx(nice):
    return nice.Context(0)


def encoded(nice, O, ctx, tw=64, th=48):
    """The reference set's ImageSet with alpha, encoded once."""
    import torch
    if (tw, th) not in _ENC:
        _ENC[tw, th] = nice.encode_set(_cuda(torch, ref(O, tw, th).imgs), tile=(tw, th), ctx=ctx, alpha=True)
    return _ENC[tw, th]


# ---- 0. what the oracle says about the reference set ----------------------------
def test_reference_set_counts(O):
    """The precondition of everything below, from the oracle alone."""
    want = {(64, 48): ([0, 12, 20, 22, 23, 29, 30], 14, 2, 14, 0),
            (50, 40): ([0, 12, 30, 32, 33, 39, 43], 28, 4, 11, 0),
            (9, 8): ([0, 345, 693, 701, 702, 837, 885], 0, 390, 495, 167)}
    for (tw, th), (first, coded, raw, constant, failed) in want.items():
        r = ref(O, tw, th)
        assert r.first == first
        assert (r.count(0), r.count(1), r.count(2), r.verify_failed) == (coded, raw, constant, failed), (tw, th)
    r = ref(O)
    assert sorted({v for k, v in zip(r.kind, r.value) if k == 2}) == [0, 17, 255]
    assert r.kind[0:12] == [2, 0, 1, 0, 2, 2, 2, 0, 2, 2, 2, 0]
    assert r.kind[20:22] == [2, 2] and r.kind[22:29] == [0] * 7       # image 2 constant, images 3 and 4 coded


# ---- 1. the range pass alone, on random bytes ------------------------------------
# members (w, h, pitch_extra, base_off): 16 bytes per lane (twice: 4 * 333 + 12 is a multiple of 16), dwords, bytes
RANGE_MIX = [(200, 136, 0, 0), (333, 211, 12, 0), (5, 7, 0, 4), (65, 1, 0, 1)]
RANGE_CASES = {"tile_64": (64, 64, RANGE_MIX), "tile_66x70": (66, 70, RANGE_MIX),
               "long_row": (1300, 8, [(1500, 9, 0, 0), (5, 7, 0, 0)])}      # a row longer than one unrolled step


@pytest.mark.parametrize("name", list(RANGE_CASES))
def test_range_matches_numpy(nice, ctx, name):
    import torch
    tw, th, members = RANGE_CASES[name]
    first = _first([(w, h) for w, h, _, _ in members], tw, th)
    n = first[-1]
    imgs = []
    for i, (w, h, _, _) in enumerate(members):
        rng = np.random.default_rng(w + 3 * h + tw + i)
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        # narrow ranges per global tile, offset per image, so that a pixel read from a neighbouring tile or image shows
        lab = first[i] + (np.arange(h)[:, None] // th) * (-(-w // tw)) + np.arange(w)[None, :] // tw
        img[:, :, 3] = ((lab * 37 + i * 11) % 200 + rng.integers(0, 9, (h, w))).astype(np.uint8)
        imgs.append(img)
    planes = np.concatenate([np_tiles(im, tw, th)[:, :, :, 3].reshape(-1, tw * th) for im in imgs])
    assert planes.shape[0] == n
    dev = [device_image(torch, im, pe, bo) for im, (_, _, pe, bo) in zip(imgs, members)]
    lo = torch.full((n + 1,), 77, dtype=torch.int32, device="cuda")
    hi = torch.full((n + 1,), 77, dtype=torch.int32, device="cuda")
    rc = nice.lib().nice_set_alpha_range_dev(
        ctx.ptr, None, _ptrs([v.data_ptr() for _, v in dev]), _u64s([w * 4 + pe for w, _, pe, _ in members]),
        _u32s([w for w, _, _, _ in members]), _u32s([h for _, h, _, _ in members]), len(members), tw, th,
        ctypes.c_void_p(lo.data_ptr()), ctypes.c_void_p(hi.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    assert lo.cpu().tolist() == planes.min(axis=1).tolist() + [77]        # (the entry past n is untouched)
    assert hi.cpu().tolist() == planes.max(axis=1).tolist() + [77]


# ---- 2. encode against the oracle --------------------------------------------------
def _check_alpha(r, a):
    n = r.n
    assert a is not None
    lens, off, kind, val = a.stream_len.numpy(), a.off.numpy(), a.kind.numpy(), a.value.numpy()
    assert kind.tolist() == r.kind
    assert val.tolist() == r.value
    assert off.shape == (n + 1,) and off[0] == 0 and np.array_equal(np.diff(off), (lens + 15) // 16 * 16)
    assert a.packed.numel() == off[n] == a.nbytes
    blob = a.packed.cpu().numpy()
    for t in range(n):
        assert blob[off[t]:off[t] + lens[t]].tobytes() == r.stored[t], (t, kind[t])
        assert not blob[off[t] + lens[t]:off[t + 1]].any(), t


@pytest.mark.parametrize("tw,th", TILES)
def test_encode_matches_oracle(nice, O, ctx, tw, th):
    iset = encoded(nice, O, ctx, tw, th)
    _check_alpha(ref(O, tw, th), iset.alpha)
    assert iset.alpha.packed.is_cuda and not iset.alpha.off.is_cuda
    assert iset.first == ref(O, tw, th).first


# ---- 3. the defining property --------------------------------------------------------
@pytest.mark.parametrize("tw,th", TILES)
def test_alpha_is_the_concatenation_of_tiled_images(nice, O, ctx, tw, th):
    """Global tile first[i] + t is tile t of encode_tiled(alpha=True) of image i alone."""
    import torch
    r = ref(O, tw, th)
    a = encoded(nice, O, ctx, tw, th).alpha
    blob, off = a.packed.cpu().numpy(), a.off.numpy()
    for i, img in enumerate(_cuda(torch, r.imgs)):
        one = nice.encode_tiled(img, tile=(tw, th), ctx=ctx, alpha=True).alpha
        lo, hi = r.first[i], r.first[i + 1]
        assert one.kind.tolist() == a.kind[lo:hi].tolist(), i
        assert one.value.tolist() == a.value[lo:hi].tolist(), i
        assert one.stream_len.tolist() == a.stream_len[lo:hi].tolist(), i
        assert (one.off + int(off[lo])).tolist() == off[lo:hi + 1].tolist(), i
        assert np.array_equal(one.packed.cpu().numpy(), blob[off[lo]:off[hi]]), i


def test_one_image_set_is_the_tiled_alpha_batch(nice, O, ctx):
    import torch
    img = torch.from_numpy(ref(O).imgs[0]).cuda()
    a = nice.encode_set([img], tile=(64, 48), ctx=ctx, alpha=True).alpha
    b = nice.encode_tiled(img, tile=(64, 48), ctx=ctx, alpha=True).alpha
    assert torch.equal(a.packed, b.packed) and torch.equal(a.off, b.off) and torch.equal(a.stream_len, b.stream_len)
    assert torch.equal(a.kind, b.kind) and torch.equal(a.value, b.value)


def test_encode_pitched_and_offset_inputs(nice, O, ctx):
    """One image per fallback mode of the range pass (and pitched 16-byte ones), in one call."""
    import torch
    r = ref(O)
    layout = [(12, 0), (0, 4), (0, 1), (32, 0), (20, 4), (0, 0)]        # (pitch_extra, base_off) per image
    dev = [device_image(torch, im, pe, bo) for im, (pe, bo) in zip(r.imgs, layout)]
    iset = nice.encode_set([v for _, v in dev], tile=(64, 48), ctx=ctx, alpha=True)
    _check_alpha(r, iset.alpha)
    plain = encoded(nice, O, ctx)
    assert torch.equal(iset.alpha.packed, plain.alpha.packed) and torch.equal(iset.packed, plain.packed)
    for (raw, _), (_, bo) in zip(dev, layout):
        assert (raw.view(-1)[:bo] == POISON).all()         # (the inputs are only read)


# ---- 4. the colour batch is untouched -----------------------------------------------
def test_colour_batch_is_untouched(nice, O, ctx):
    import torch
    r = ref(O)
    plain = nice.encode_set(_cuda(torch, r.imgs), tile=(64, 48), ctx=ctx)
    assert plain.alpha is None
    both = encoded(nice, O, ctx)
    assert torch.equal(plain.packed, both.packed) and torch.equal(plain.off, both.off)
    assert torch.equal(plain.stream_len, both.stream_len) and torch.equal(plain.kind, both.kind)
    for im, out in zip(r.imgs, nice.decode_set(plain, ctx=ctx)):          # decodes as before: RGB and the fill
        got = out.cpu().numpy()
        assert np.array_equal(got[:, :, :3], im[:, :, :3]) and (got[:, :, 3] == 255).all()


# ---- 5. round trips ------------------------------------------------------------------
@pytest.mark.parametrize("tw,th", TILES)
def test_round_trip(nice, O, ctx, tw, th):
    r = ref(O, tw, th)
    iset = encoded(nice, O, ctx, tw, th)
    outs = nice.decode_set(iset, ctx=ctx)
    assert len(outs) == K
    for im, out in zip(r.imgs, outs):
        assert tuple(out.shape) == im.shape and np.array_equal(out.cpu().numpy(), im)
    for im, out in zip(r.imgs, nice.decode_set(iset, flags=0, ctx=ctx)):       # the fill flag is irrelevant
        assert np.array_equal(out.cpu().numpy(), im)
    for i, out in zip([4, 0], nice.decode_set(iset, images=[4, 0], ctx=ctx)):
        assert np.array_equal(out.cpu().numpy(), r.imgs[i])
    for im, out in zip(r.imgs, nice.decode_set(iset, out_channels=3, ctx=ctx)):
        assert np.array_equal(out.cpu().numpy(), im[:, :, :3])


# ---- 6. windows -----------------------------------------------------------------------
# at 64 x 48: x0 % 4 nonzero and zero across tile edges, inside the constant tile 0 and the raw tile 2 of image 0,
# inside image 3, the last pixels of images 0 and 1, two windows sharing tile (1, 1) of image 4, a constant image
WINDOWS = [(0, 61, 43, 9, 11), (0, 60, 40, 80, 30), (0, 4, 4, 40, 30), (0, 130, 2, 48, 40), (3, 1, 2, 3, 4),
           (0, 199, 119, 1, 1), (1, 255, 95, 1, 1), (4, 60, 40, 20, 20), (4, 70, 50, 30, 15), (5, 0, 0, 64, 48),
           (1, 3, 5, 250, 90)]


@pytest.mark.parametrize("tw,th", [(64, 48), (50, 40)])
def test_windows_into_strided_views(nice, O, ctx, tw, th):
    """Row-strided outputs with a poisoned lead and slack: 4 pixels of lead in
    rows of rw + 8 pixels, so a window with x0 % 4 == 0 and rw % 4 == 0 takes
    the 16-byte path (64 x 48) and the others the byte path, in one launch."""
    import torch
    r = ref(O, tw, th)
    iset = encoded(nice, O, ctx, tw, th)
    if (tw, th) == (64, 48):
        k = r.slot_kinds([WINDOWS[2]]), r.slot_kinds([WINDOWS[3]])
        assert k == ([2], [1])
    bigs = [torch.full((rh + 2, rw + 8, 4), POISON, dtype=torch.uint8, device="cuda") for _, _, _, rw, rh in WINDOWS]
    views = [b[1:-1, 4:-4] for b in bigs]
    back = nice.decode_set(iset, windows=WINDOWS, out=views, ctx=ctx)
    assert all(a is b for a, b in zip(back, views))
    for (i, x0, y0, rw, rh), big in zip(WINDOWS, bigs):
        got = big.cpu().numpy()
        assert np.array_equal(got[1:-1, 4:-4], r.imgs[i][y0:y0 + rh, x0:x0 + rw]), (i, x0, y0, rw, rh)
        got[1:-1, 4:-4] = POISON
        assert (got == POISON).all(), (i, x0, y0, rw, rh)
    for (i, x0, y0, rw, rh), out in zip(WINDOWS, nice.decode_set(iset, windows=WINDOWS, ctx=ctx)):   # no out
        assert np.array_equal(out.cpu().numpy(), r.imgs[i][y0:y0 + rh, x0:x0 + rw])


# (rw, rh): 9 x 11 is 396 bytes per window in rows of 36: bases 16- or 4-byte aligned, the pitch never 16-byte
# aligned (dword descriptors: byte stores); 32 x 32 is 16-byte aligned throughout, so x0 % 4 picks the path
@pytest.mark.parametrize("rw,rh", [(9, 11), (32, 32)])
def test_crop_batch(nice, O, ctx, rw, rh):
    import torch
    r = ref(O)
    iset = encoded(nice, O, ctx)
    at = [(0, 60, 40), (0, 61, 3), (0, 128, 8), (1, 100, 30), (1, 224, 64), (4, 0, 0), (4, 98, 38), (5, 32, 16),
          (0, 168, 88), (4, 41, 17)]
    crops = [(i, x0, y0, rw, rh) for i, x0, y0 in at]
    out = torch.full((len(crops), rh, rw, 4), POISON, dtype=torch.uint8, device="cuda")
    assert nice.decode_set(iset, windows=crops, out=out, ctx=ctx) is out
    got = out.cpu().numpy()
    for j, (i, x0, y0, _, _) in enumerate(crops):
        assert np.array_equal(got[j], r.imgs[i][y0:y0 + rh, x0:x0 + rw]), j


# ---- 7. the alpha pass alone ------------------------------------------------------------
def last_set_alpha(nice, ctx):
    L = nice.lib()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.nice_test_last_set_alpha.argtypes = [ctypes.c_void_p, u32p, u32p, u32p]
    v = [ctypes.c_uint32() for _ in range(3)]
    assert L.nice_test_last_set_alpha(ctx.ptr, *[ctypes.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


def _alpha_alone(nice, ctx, iset, windows, ptrs, pitches, alpha=None):
    """nice_decode_set_alpha_dev alone on the windows; the statuses."""
    import torch
    a = iset.alpha if alpha is None else alpha
    n = iset.first[-1]
    ns = nice.set_select(iset.widths, iset.heights, iset.tile_w, iset.tile_h, windows)[-1]
    status = torch.full((ns,), 99, dtype=torch.int32, device="cuda")
    tabs = [a.off.contiguous(), a.stream_len.contiguous(), a.kind.contiguous(), a.value.contiguous()]
    rc = nice.lib().nice_decode_set_alpha_dev(
        ctx.ptr, None, ctypes.c_void_p(a.packed.data_ptr() if a.packed.numel() else None), int(a.off[n]),
        *[ctypes.c_void_p(t.data_ptr()) for t in tabs], _u32s(iset.widths), _u32s(iset.heights), len(iset.widths),
        iset.tile_w, iset.tile_h, _u32s([v for wdw in windows for v in wdw]), _ptrs(ptrs), _u64s(pitches),
        len(windows), ctypes.c_void_p(status.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    return status.cpu().tolist()


ALONE = [(0, 0, 0, 200, 120), (1, 0, 0, 256, 96), (0, 60, 40, 80, 30), (0, 61, 43, 9, 11), (3, 0, 0, 5, 7),
         (4, 4, 4, 120, 60), (5, 8, 8, 40, 30), (2, 0, 0, 65, 1)]


# (lead bytes, pitch slack): window rows 16-byte aligned (the 16-byte read-modify-write where x0 % 4 == 0) or not
@pytest.mark.parametrize("lead,slack", [(16, 0), (20, 0), (16, 4), (17, 3)])
@pytest.mark.parametrize("tw,th", [(64, 48), (50, 40)])
def test_alpha_pass_writes_only_alpha(nice, O, ctx, tw, th, lead, slack):
    """The alpha call alone on patterned tensors: byte +3 of the windows'
    pixels becomes the images' alpha; the windows' colour bytes and every byte
    around the windows stay."""
    import torch
    r = ref(O, tw, th)
    iset = encoded(nice, O, ctx, tw, th)
    befores, bigs, ptrs, pitches = [], [], [], []
    for j, (i, x0, y0, rw, rh) in enumerate(ALONE):
        pitch = (rw * 4 + 15) // 16 * 16 + 32 + slack
        before = np.roll(_pattern((rh + 2, pitch)), j)
        big = torch.from_numpy(before).cuda()
        assert big.data_ptr() % 16 == 0
        befores.append(before)
        bigs.append(big)
        ptrs.append(big.data_ptr() + pitch + lead)
        pitches.append(pitch)
    st = _alpha_alone(nice, ctx, iset, ALONE, ptrs, pitches)
    assert st == [0] * len(st)
    kinds = r.slot_kinds(ALONE)
    assert last_set_alpha(nice, ctx) == (kinds.count(0), kinds.count(1), kinds.count(2))
    for (i, x0, y0, rw, rh), before, big in zip(ALONE, befores, bigs):
        want = before.copy()
        want[1:1 + rh, lead:lead + rw * 4].reshape(rh, rw, 4)[:, :, 3] = r.imgs[i][y0:y0 + rh, x0:x0 + rw, 3]
        assert np.array_equal(big.cpu().numpy(), want), (i, x0, y0, lead, slack)


# ---- 8. selection ---------------------------------------------------------------------------
def test_selection_counts_and_constant_windows(nice, O):
    """The slots by kind equal the oracle's kinds of the touched tiles; a
    window inside constant tiles decodes no stream."""
    import torch
    ctx = nice.Context(0)
    r = ref(O)
    iset = encoded(nice, O, ctx)
    nice.decode_set(iset, windows=WINDOWS, ctx=ctx)
    kinds = r.slot_kinds(WINDOWS)
    assert last_set_alpha(nice, ctx) == (kinds.count(0), kinds.count(1), kinds.count(2))
    assert kinds.count(0) > 0 and kinds.count(1) > 0 and kinds.count(2) > 0
    flat = [(0, 4, 4, 40, 30), (5, 0, 0, 64, 48), (2, 0, 0, 65, 1), (0, 10, 50, 100, 60)]
    assert set(r.slot_kinds(flat)) == {2}
    outs = [torch.full((rh, rw, 4), POISON, dtype=torch.uint8, device="cuda") for _, _, _, rw, rh in flat]
    L = nice.lib()
    L.nice_ctx_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.nice_ctx_set_timing(ctx.ptr, 1) == 0
    try:
        _timing(nice, ctx)
        st = _alpha_alone(nice, ctx, iset, flat, [o.data_ptr() for o in outs], [rw * 4 for _, _, _, rw, _ in flat])
        assert _timing(nice, ctx)[PH_DEC_TABLES] == 0                  # no decode was launched
    finally:
        L.nice_ctx_set_timing(ctx.ptr, 0)
    assert st == [0] * 8 and last_set_alpha(nice, ctx) == (0, 0, 8)
    for (i, x0, y0, rw, rh), o in zip(flat, outs):
        got = o.cpu().numpy()
        assert (got[:, :, :3] == POISON).all() and np.array_equal(got[:, :, 3], r.imgs[i][y0:y0 + rh, x0:x0 + rw, 3])


# ---- 9. launch counts depend on neither K nor M ----------------------------------------------
def test_launch_counts_do_not_depend_on_images_or_windows(nice, O):
    import torch
    ctx = nice.Context(0)
    imgs = _cuda(torch, ref(O).imgs)
    L = nice.lib()
    L.nice_ctx_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.nice_ctx_set_timing(ctx.ptr, 1) == 0
    try:
        _timing(nice, ctx)
        plain = nice.encode_set(imgs, tile=(64, 48), ctx=ctx)
        enc_plain = _timing(nice, ctx)
        six = nice.encode_set(imgs, tile=(64, 48), ctx=ctx, alpha=True)
        enc_six = _timing(nice, ctx)
        nice.encode_set(imgs + imgs, tile=(64, 48), ctx=ctx, alpha=True)
        enc_twelve = _timing(nice, ctx)
        # the colour encode and its verify decode, then those of the alpha, whatever K is
        assert enc_plain[PH_ENC_CLASSIFY] > 0 and enc_plain[PH_DEC_TABLES] > 0
        assert enc_six[PH_ENC_CLASSIFY] > enc_plain[PH_ENC_CLASSIFY]
        assert enc_six[PH_DEC_TABLES] > enc_plain[PH_DEC_TABLES]
        assert enc_twelve[PH_ENC_CLASSIFY] == enc_six[PH_ENC_CLASSIFY]
        assert enc_twelve[PH_DEC_TABLES] == enc_six[PH_DEC_TABLES]
        nice.decode_set(plain, windows=WINDOWS, ctx=ctx)
        dec_plain = _timing(nice, ctx)
        nice.decode_set(six, windows=WINDOWS, ctx=ctx)
        dec_m = _timing(nice, ctx)
        nice.decode_set(six, windows=WINDOWS + WINDOWS, ctx=ctx)
        dec_2m = _timing(nice, ctx)
        assert dec_plain[PH_DEC_TABLES] > 0 and dec_m[PH_ENC_CLASSIFY] == 0
        assert dec_m[PH_DEC_TABLES] > dec_plain[PH_DEC_TABLES] and dec_2m[PH_DEC_TABLES] == dec_m[PH_DEC_TABLES]
    finally:
        L.nice_ctx_set_timing(ctx.ptr, 0)


# ---- 10. the opaque set -----------------------------------------------------------------------
def test_opaque_set_costs_the_range_pass_only(nice, O):
    import torch
    ctx = nice.Context(0)
    imgs = [im.copy() for im in ref(O).imgs]
    for im in imgs:
        im[:, :, 3] = 255
    dev = _cuda(torch, imgs)
    L = nice.lib()
    L.nice_ctx_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.nice_ctx_set_timing(ctx.ptr, 1) == 0
    try:
        _timing(nice, ctx)
        plain = nice.encode_set(dev, tile=(64, 48), ctx=ctx)
        enc_plain = _timing(nice, ctx)
        iset = nice.encode_set(dev, tile=(64, 48), ctx=ctx, alpha=True)
        enc_alpha = _timing(nice, ctx)
        a = iset.alpha
        assert a.kind.tolist() == [2] * 30 and a.value.tolist() == [255] * 30
        assert a.packed.numel() == 0 and a.off.tolist() == [0] * 31 and a.stream_len.tolist() == [0] * 30
        assert enc_plain[PH_ENC_CLASSIFY] > 0 and enc_alpha == enc_plain      # no encode, no decode for the alpha
        outs_plain = nice.decode_set(plain, ctx=ctx)
        dec_plain = _timing(nice, ctx)
        outs = nice.decode_set(iset, flags=0, ctx=ctx)
        dec_alpha = _timing(nice, ctx)
        assert dec_plain[PH_DEC_TABLES] > 0 and dec_alpha == dec_plain
        for im, o, p in zip(imgs, outs, outs_plain):
            assert np.array_equal(o.cpu().numpy(), im) and torch.equal(o, p)
    finally:
        L.nice_ctx_set_timing(ctx.ptr, 0)


# ---- 11. errors ----------------------------------------------------------------------------------
def test_rgb_images_are_refused(nice, O, ctx):
    import torch
    imgs = _cuda(torch, [im[:, :, :3] for im in ref(O).imgs])
    with pytest.raises(nice.NiceError) as e:
        nice.encode_set(imgs, tile=(64, 48), ctx=ctx, alpha=True)
    assert e.value.code == E_ARG


def test_encode_capacity(nice, O, ctx):
    """Too small a buffer: NICE_E_CAPACITY, aoff[n] the size needed, nothing at or past the capacity written."""
    import torch
    r = ref(O)
    need = encoded(nice, O, ctx).alpha.nbytes
    imgs = _cuda(torch, r.imgs)
    n = r.n
    for cap, want in ((need - 16, E_CAPACITY), (need, 0)):
        buf = torch.full((need + 64,), POISON, dtype=torch.uint8, device="cuda")
        off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        lens = torch.zeros(n, dtype=torch.int64, device="cuda")
        kind = torch.zeros(n, dtype=torch.uint8, device="cuda")
        val = torch.zeros(n, dtype=torch.uint8, device="cuda")
        status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        rc = nice.lib().nice_encode_set_alpha_dev(
            ctx.ptr, None, _ptrs([t.data_ptr() for t in imgs]), _u64s([w * 4 for w, _ in r.shapes]),
            _u32s([w for w, _ in r.shapes]), _u32s([h for _, h in r.shapes]), K, 64, 48,
            ctypes.c_void_p(buf.data_ptr()), cap, *[ctypes.c_void_p(t.data_ptr()) for t in (off, lens, kind, val, status)])
        assert rc == 0
        torch.cuda.synchronize()
        assert int(status.cpu()[0]) == want
        assert int(off.cpu()[n]) == need
        assert bool((buf[cap:] == POISON).all())
        assert kind.cpu().tolist() == r.kind
    ws, hs = [w for w, _ in r.shapes], [h for _, h in r.shapes]
    assert nice.set_alpha_bound(ws, hs, 64, 48) == n * ((max(nice.encode_bound(22, 48), 64 * 48) + 15) // 16 * 16)
    assert nice.set_alpha_bound(ws, hs, 1, 48) == 0 and nice.set_alpha_bound(ws, hs[:-1], 64, 48) == 0


def test_damaged_alpha_tile_fails_alone(nice, O, ctx):
    """The first bytes of one coded alpha stream zeroed: every slot of that
    tile fails, in every window that touches it, and keeps the fill; every
    other pixel is right and the colour statuses are all OK."""
    r = ref(O)
    iset = encoded(nice, O, ctx)
    a = iset.alpha
    bad_t = 1                                                 # the disc of image 0, a coded tile
    assert r.kind[bad_t] == 0
    packed = a.packed.clone()
    packed[int(a.off[bad_t]):int(a.off[bad_t]) + 16] = 0
    hurt = dataclasses.replace(iset, alpha=dataclasses.replace(a, packed=packed))
    windows = [(i, 0, 0, w, h) for i, (w, h) in enumerate(r.shapes)] + [(0, 70, 10, 20, 20), (0, 60, 40, 80, 30)]
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set(hurt, windows=windows, ctx=ctx)
    ast = e.value.alpha_statuses
    hit = [p for p, (j, ti) in enumerate((j, ti) for j, (i, x0, y0, rw, rh) in enumerate(windows)
                                         for ti in _touched(*r.shapes[i], 64, 48, x0, y0, rw, rh))
           if windows[j][0] == 0 and ti == bad_t]
    assert len(hit) == 3 and len(ast) == 30 + 1 + 6
    assert [p for p, s in enumerate(ast) if s != 0] == hit
    assert e.value.statuses == [0] * len(ast)
    for (i, x0, y0, rw, rh), out in zip(windows, e.value.out):
        want = r.imgs[i].copy()
        if i == 0:
            want[0:48, 64:128, 3] = 255                       # what the colour pass wrote there
        assert np.array_equal(out.cpu().numpy(), want[y0:y0 + rh, x0:x0 + rw]), (i, x0, y0)
    # a kind of 3 in the host table: that slot alone
    kind = a.kind.clone()
    kind[r.first[4] + 4] = 3
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set(dataclasses.replace(iset, alpha=dataclasses.replace(a, kind=kind)), images=[4, 3], ctx=ctx)
    assert e.value.alpha_statuses == [0, 0, 0, 0, E_FORMAT, 0, 0] and e.value.statuses == [0] * 7
    got = e.value.out[0].cpu().numpy()
    want = r.imgs[4].copy()
    want[48:, 64:128, 3] = 255
    assert np.array_equal(got, want) and np.array_equal(e.value.out[1].cpu().numpy(), r.imgs[3])


def test_nothing_left_to_decode(nice, O, ctx):
    """Every tile's kind outside the format, in both batches ({100 x 70,
    33 x 20} at 64 x 48, 5 tiles): decode_set's two passes and
    decode_set_tensor refuse every slot on the host, nothing but the window
    descriptors is uploaded, nothing is decoded, the outputs keep their poison,
    the counters are zero, and the context then decodes the sound set exactly."""
    import torch
    from test_sets import last_set
    shapes, tw, th, n = [(100, 70), (33, 20)], 64, 48, 5
    rng = np.random.default_rng(6)
    imgs = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for w, h in shapes]
    iset = nice.encode_set(_cuda(torch, imgs), tile=(tw, th), ctx=ctx, alpha=True)
    assert iset.first == [0, 4, 5]
    hurt = dataclasses.replace(iset, kind=torch.full((n,), 7, dtype=torch.uint8),
                               alpha=dataclasses.replace(iset.alpha, kind=torch.full((n,), 3, dtype=torch.uint8)))
    whole = [(i, 0, 0, w, h) for i, (w, h) in enumerate(shapes)]
    for windows, m in ((whole, 5), ([(0, 60, 40, 30, 20), (1, 3, 2, 9, 11), (0, 60, 40, 30, 20)], 9), ([(1, 0, 0, 1, 1)], 1)):
        outs = [torch.full((rh, rw, 4), POISON, dtype=torch.uint8, device="cuda") for _, _, _, rw, rh in windows]
        nice.decode_set(iset, images=[1], ctx=ctx)                # (the counters start from a sound decode's)
        assert sum(last_set(nice, ctx)) == 1 and sum(last_set_alpha(nice, ctx)) == 1
        with pytest.raises(nice.NiceError) as e:
            nice.decode_set(hurt, windows=windows, out=outs, ctx=ctx)
        assert e.value.statuses == [E_FORMAT] * m and e.value.alpha_statuses == [E_FORMAT] * m
        assert all(bool((o == POISON).all()) for o in outs)
        assert last_set(nice, ctx) == (0, 0) and last_set_alpha(nice, ctx) == (0, 0, 0)
        touts = [torch.full((3, rh, rw), -768.0, dtype=torch.float16, device="cuda") for _, _, _, rw, rh in windows]
        nice.decode_set_tensor(iset, images=[1], ctx=ctx)
        assert sum(last_set(nice, ctx)) == 1
        with pytest.raises(nice.NiceError) as e:
            nice.decode_set_tensor(hurt, windows=windows, out=touts, ctx=ctx)
        assert e.value.statuses == [E_FORMAT] * m
        assert all(bool((o == -768.0).all()) for o in touts)
        assert last_set(nice, ctx) == (0, 0)
    for got, im in zip(nice.decode_set(iset, ctx=ctx), imgs):
        assert np.array_equal(got.cpu().numpy(), im)
    assert sum(last_set(nice, ctx)) == n and sum(last_set_alpha(nice, ctx)) == n
    scale = (1.0, 1.0, 1.0)
    for got, im in zip(nice.decode_set_tensor(iset, dtype=torch.float32, scale=scale, ctx=ctx), imgs):
        assert np.array_equal(got.cpu().numpy(), im[:, :, :3].transpose(2, 0, 1).astype(np.float32))


# ---- 12. container and command line -------------------------------------------------------------------
def test_container_round_trip(nice, O, ctx, tmp_path):
    import torch
    r = ref(O)
    iset = encoded(nice, O, ctx)
    path = str(tmp_path / "set.nices")
    nice.save_set(path, iset)
    back = nice.load_set(path, device="cuda")
    assert back.alpha.packed.is_cuda and torch.equal(back.alpha.packed, iset.alpha.packed)
    assert torch.equal(back.alpha.kind, iset.alpha.kind) and torch.equal(back.alpha.value, iset.alpha.value)
    assert torch.equal(back.packed, iset.packed) and back.first == iset.first
    for im, out in zip(r.imgs, nice.decode_set(back, ctx=ctx)):
        assert np.array_equal(out.cpu().numpy(), im)
    plain = dataclasses.replace(iset, alpha=None)              # a version 1 file decodes to the same RGB as before
    nice.save_set(path, plain)
    v1 = nice.load_set(path, device="cuda")
    assert v1.alpha is None
    for x, y in zip(nice.decode_set(v1, ctx=ctx), nice.decode_set(plain, ctx=ctx)):
        assert torch.equal(x, y)


def test_cli_directory_set_directory(nice, O, tmp_path):
    """(directory of RGBA PNGs -> --set --alpha --tile 64x48 -> .nices -> directory of RGBA PNGs, and --index)"""
    png = importlib.import_module(PKG_NAME + ".png")
    r = ref(O)
    src = tmp_path / "in"
    src.mkdir()
    for i, im in enumerate(r.imgs):
        png.write_png(str(src / f"img{i}.png"), im.reshape(-1), im.shape[1], im.shape[0], 4)
    run = subprocess.run([sys.executable, CLI, "--set", str(src), str(tmp_path / "out"), "--tile", "64x48", "--alpha"],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "images: 6 tiles: 30 raw:" in run.stdout and "alpha tiles: coded: 14 raw: 2 constant: 14" in run.stdout
    assert nice.load_set(str(tmp_path / "out.nices")).alpha.kind.tolist() == r.kind
    run = subprocess.run([sys.executable, CLI, str(tmp_path / "out.nices"), str(tmp_path / "back")],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert sorted(os.listdir(tmp_path / "back")) == [f"{i:06d}.png" for i in range(K)]
    for i, im in enumerate(r.imgs):
        got, gw, gh, gc = png.read_png(str(tmp_path / "back" / f"{i:06d}.png"))
        assert (gw, gh, gc) == (im.shape[1], im.shape[0], 4) and np.array_equal(got.reshape(im.shape), im), i
    run = subprocess.run([sys.executable, CLI, str(tmp_path / "out.nices"), str(tmp_path / "one.png"), "--index", "4"],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got, gw, gh, gc = png.read_png(str(tmp_path / "one.png"))
    assert (gw, gh, gc) == (130, 70, 4) and np.array_equal(got.reshape(70, 130, 4), r.imgs[4])
    rgb = tmp_path / "rgb"
    rgb.mkdir()
    png.write_png(str(rgb / "a.png"), np.ascontiguousarray(r.imgs[3][:, :, :3]).reshape(-1), 5, 7, 3)
    run = subprocess.run([sys.executable, CLI, "--set", str(rgb), str(tmp_path / "no"), "--tile", "64x48", "--alpha"],
                         capture_output=True, text=True)
    assert run.returncode == 2 and "RGBA" in run.stderr
