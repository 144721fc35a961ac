"""Image sets, resized tensor output (include/nice.h, "image sets: resized
tensor output") on the GPU: the resize kernel alone on random bytes in
hand-built slots, then decode_set_resized end to end on the reference set of
tests/test_sets.py, then the host refusals.

The reference is the numpy model of tests/test_sets_resize_cpu.py (positions in
Python integers, the accumulator in int64, the element as the single rounding
of the exact rational).  Every comparison is bit for bit on the integer view;
poisoned guards surround every output, and an element with a tap in a failed or
unreadable slot must keep the poison."""
import ctypes
import dataclasses

import numpy as np
import pytest

from test_sets import (CROPS, K, PH_DEC_TABLES, _cuda, _random_image, _slot_counts, _timing, _touched, encoded, last_set,
                       ref)
from test_sets_tensor import (BF16, CROP_FLIPS, DTYPES, F16, F32, INTERLEAVED, PLANAR, POISON, POISON_BITS, _merge_tensor,
                              _tdtype, bits_of, expect_bits, holds_halfway, lut_bits, plant_halfway)
from test_sets_tensor_cpu import const_sets
from test_sets_resize_cpu import model_bits, positions

pytestmark = pytest.mark.gpu

E_ARG = -1
KIND_DENSE, KIND_RAW, KIND_NONE = 0, 1, 3


@pytest.fixture(scope="module")
def ctx(nice):
    return nice.Context(0)


def garbage_tiles(img, tw, th):
    """[h, w, 4] -> [n, th, tw, 4], tile t = ty * nx + tx; what lies outside the
    image is noise, not the clamp rule's padding: a resized window reads no
    pixel outside itself."""
    h, w, c = img.shape
    nx, ny = -(-w // tw), -(-h // th)
    big = np.random.default_rng(w + h).integers(0, 256, (ny * th, nx * tw, c), dtype=np.uint8)
    big[:h, :w] = img
    return np.ascontiguousarray(big.reshape(ny, th, nx, tw, c).transpose(0, 2, 1, 3, 4).reshape(nx * ny, th, tw, c))


def tap_tiles_hit(wdw, size, flip, tw, th, nx, bad_tiles):
    """[oh, ow] bool: the elements of the resized window with a tap in one of bad_tiles (tile indices of its image)."""
    _, x0, y0, rw, rh = wdw
    oh, ow = size
    i0, i1, _ = positions(rw, ow, flip)
    j0, j1, _ = positions(rh, oh)
    hit = np.zeros((oh, ow), bool)
    for jj in (j0, j1):
        for ii in (i0, i1):
            t = ((y0 + jj) // th)[:, None] * nx + ((x0 + ii) // tw)[None, :]
            hit |= np.isin(t, list(bad_tiles))
    return hit


def expect_window(img, wdw, size, flip, consts, dtype, tw, th, poison, bad_tiles=()):
    _, x0, y0, rw, rh = wdw
    want = model_bits(img[y0:y0 + rh, x0:x0 + rw], size[0], size[1], flip, consts[0], consts[1], dtype).copy()
    if bad_tiles:
        hit = tap_tiles_hit(wdw, size, flip, tw, th, -(-img.shape[1] // tw), bad_tiles)
        want[:, hit] = poison
    return want


# ---- 1. the kernel alone ---------------------------------------------------------------------
def _resize(nice, ctx, imgs, tw, th, windows, size, dt, layout, leads, flips, consts, kinds=None, raw_lead=0,
            failed=(), odd_pitch=(), no_status=False):
    """Every (window, tile) slot of `windows`, in position order, through
    nice_set_resize_tensor_dev into one poisoned buffer per window, guarded as
    test_sets_tensor._merge_tensor guards its own; window j's first element is
    leads[j] elements past a 16-byte boundary, and its row pitch is odd where
    j is in odd_pitch.  kinds[p]: KIND_DENSE (4 bytes per pixel, byte +3
    noise), KIND_RAW (3 bytes per pixel, raw_lead bytes past a multiple of 16)
    or KIND_NONE; failed: positions with a nonzero status.  Returns each
    window's bits [3, oh, ow] and the poison."""
    import torch
    oh, ow = size
    es = 4 if dt == F32 else 2
    idt = torch.int32 if es == 4 else torch.int16
    poison = POISON_BITS[es]
    rgba = [np.concatenate([im[:, :, :3], _random_image(im.shape[1], im.shape[0], 1, 99)], axis=2) for im in imgs]
    tiles = [garbage_tiles(im, tw, th) for im in rgba]
    slots = [(j, ti) for j, (i, x0, y0, rw, rh) in enumerate(windows)
             for ti in _touched(imgs[i].shape[1], imgs[i].shape[0], tw, th, x0, y0, rw, rh)]
    ns = len(slots)
    kinds = [KIND_DENSE] * ns if kinds is None else list(kinds)
    assert len(kinds) == ns
    dstride = (tw * th * 4 + 15) // 16 * 16
    rstride = (tw * th * 3 + 15) // 16 * 16 + 16
    dense = np.full((max(kinds.count(KIND_DENSE), 1), dstride), 0xA5, np.uint8)
    raw = np.full(kinds.count(KIND_RAW) * rstride + 32, 0xA5, np.uint8)
    src, nd, nr = [], 0, 0
    for (j, ti), kind in zip(slots, kinds):
        data = tiles[windows[j][0]][ti]
        if kind == KIND_DENSE:
            dense[nd, :tw * th * 4] = data.reshape(-1)
            src.append((KIND_DENSE << 62) | nd)
            nd += 1
        elif kind == KIND_RAW:
            off = nr * rstride + raw_lead
            raw[off:off + tw * th * 3] = data[:, :, :3].reshape(-1)
            src.append((KIND_RAW << 62) | off)
            nr += 1
        else:
            src.append(KIND_NONE << 62)
    d_dense, d_raw = torch.from_numpy(dense).cuda(), torch.from_numpy(raw).cuda()
    assert d_dense.data_ptr() % 16 == 0 and d_raw.data_ptr() % 16 == 0
    d_src = torch.from_numpy(np.array(src, np.uint64).view(np.int64)).cuda()
    d_st = torch.tensor([-5 if p in failed else 0 for p in range(ns)], dtype=torch.int32, device="cuda")
    bigs, ptrs, rps, pps, where = [], [], [], [], []
    for j, lead in enumerate(leads):
        n_el = ow if layout == PLANAR else 3 * ow
        row = (n_el + 7) // 8 * 8 + 24 + (1 if j in odd_pitch else 0)
        rows = oh + 3                                        # a guard row above, two below (between planes)
        big = torch.full((3 if layout == PLANAR else 1, rows, row), poison, dtype=idt, device="cuda")
        assert big.data_ptr() % 16 == 0
        bigs.append(big)
        ptrs.append(big.data_ptr() + (row + 8 + lead + (7 if j in odd_pitch else 0)) * es)   # (the first row starts at a multiple of 8 + lead)
        rps.append(row)
        pps.append(rows * row)
        where.append((slice(1, 1 + oh), slice(8 + lead + (7 if j in odd_pitch else 0),
                                              8 + lead + (7 if j in odd_pitch else 0) + n_el)))
    scale, bias = consts
    m = len(windows)
    rc = nice.lib().nice_set_resize_tensor_dev(
        ctx.ptr, None, ctypes.c_void_p(d_dense.data_ptr()), dstride, ctypes.c_void_p(d_raw.data_ptr()),
        ctypes.c_void_p(d_src.data_ptr()), None if no_status else ctypes.c_void_p(d_st.data_ptr()),
        (ctypes.c_uint32 * len(imgs))(*[im.shape[1] for im in imgs]),
        (ctypes.c_uint32 * len(imgs))(*[im.shape[0] for im in imgs]), len(imgs), tw, th,
        (ctypes.c_uint32 * (5 * m))(*[v for wdw in windows for v in wdw]),
        (ctypes.c_uint8 * m)(*[1 if f else 0 for f in flips]), ow, oh, (ctypes.c_void_p * m)(*ptrs),
        (ctypes.c_uint64 * m)(*rps), (ctypes.c_uint64 * m)(*pps) if layout == PLANAR else None, m, dt, layout,
        (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias))
    assert rc == 0
    torch.cuda.synchronize()
    outs = []
    for wdw, big, (ys, xs) in zip(windows, bigs, where):
        got = big.cpu().numpy()
        win = got[:, ys, xs].copy()
        outs.append(win if layout == PLANAR else win.reshape(oh, ow, 3).transpose(2, 0, 1))
        got[:, ys, xs] = poison
        assert (got == poison).all(), wdw
    return outs, poison


# a 40 x 30 image (5 x 5 tiles of 8 x 6) and a 37 x 29 one whose last tiles are partial
SHAPES = [(40, 30), (37, 29)]
WINDOWS = [(0, 1, 1, 6, 4),          # inside one tile
           (0, 6, 4, 8, 6),          # 2 x 2 tiles
           (0, 9, 7, 20, 12),        # 3 x 3 tiles
           (0, 13, 11, 1, 1),        # one pixel
           (0, 15, 2, 1, 9),         # one pixel wide
           (0, 3, 17, 11, 1),        # one pixel high
           (1, 30, 22, 7, 7),        # ends in the image's last, partial tile
           (1, 0, 0, 37, 29),        # a whole image
           (0, 4, 4, 16, 12)]        # 12 x 16 is its own size, 6 x 8 halves it
LEADS = [0, 1, 3, 4, 2, 0, 4, 0, 0]                       # elements past a 16-byte boundary: every store width, and none
ODD = (5, 7)                                               # windows with an odd row pitch: element by element
FLIPS = [j % 2 for j in range(len(WINDOWS))]
# enlarging most windows and the last one's own size; halving it, reducing the whole image 4.8 and 4.6 times;
# one element; one column; odd sizes
SIZES = [(12, 16), (6, 8), (1, 1), (5, 1), (9, 23)]


def _images():
    return [_random_image(w, h, 3, i) for i, (w, h) in enumerate(SHAPES)]


def _check(nice, outs, poison, imgs, windows, size, flips, consts, dtype, tw, th, bad=None):
    for j, (wdw, got) in enumerate(zip(windows, outs)):
        want = expect_window(imgs[wdw[0]], wdw, size, flips[j], consts, dtype, tw, th, poison,
                             () if bad is None else bad.get(j, ()))
        assert np.array_equal(got, want), (j, wdw, size)


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("dt", [F32, F16, BF16])
@pytest.mark.parametrize("size", SIZES)
def test_resize_matches_model(nice, ctx, size, dt, layout):
    imgs = _images()
    consts = const_sets(nice)["imagenet"]
    outs, poison = _resize(nice, ctx, imgs, 8, 6, WINDOWS, size, dt, layout, LEADS, FLIPS, consts, odd_pitch=ODD)
    _check(nice, outs, poison, imgs, WINDOWS, size, FLIPS, consts, DTYPES[dt], 8, 6)


@pytest.mark.parametrize("dt,layout,size", [(F16, PLANAR, (12, 16)), (F32, INTERLEAVED, (7, 70)), (BF16, PLANAR, (33, 5))])
def test_resize_other_tile_size(nice, ctx, dt, layout, size):
    """Tiles of 16 x 8, no status column, the other constants; an output row longer than a wave has lanes."""
    imgs = _images()
    consts = const_sets(nice)["odd"]
    flips = [1 - f for f in FLIPS]
    outs, poison = _resize(nice, ctx, imgs, 16, 8, WINDOWS, size, dt, layout, LEADS, flips, consts, no_status=True)
    _check(nice, outs, poison, imgs, WINDOWS, size, flips, consts, DTYPES[dt], 16, 8)


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("raw_lead", [0, 1, 5])
def test_resize_raw_and_dense_slots_mixed(nice, ctx, raw_lead, layout):
    """Every third slot raw, 3 bytes per pixel: inside the windows of several
    tiles one element's taps come from both kinds; the values are those of
    dense slots."""
    imgs = _images()
    consts = const_sets(nice)["imagenet"]
    ns = sum(len(_touched(SHAPES[i][0], SHAPES[i][1], 8, 6, x0, y0, rw, rh)) for i, x0, y0, rw, rh in WINDOWS)
    kinds = [KIND_RAW if p % 3 == 1 else KIND_DENSE for p in range(ns)]
    assert set(kinds[1:5]) == {KIND_DENSE, KIND_RAW}                     # the 2 x 2 window (positions 1..4) mixes
    for size in ((12, 16), (9, 23)):
        outs, poison = _resize(nice, ctx, imgs, 8, 6, WINDOWS, size, BF16, layout, LEADS, FLIPS, consts, kinds=kinds,
                               raw_lead=raw_lead)
        _check(nice, outs, poison, imgs, WINDOWS, size, FLIPS, consts, "bfloat16", 8, 6)
    kinds = [KIND_RAW] * ns
    outs, poison = _resize(nice, ctx, imgs, 8, 6, WINDOWS, (6, 8), F16, layout, LEADS, FLIPS, consts, kinds=kinds,
                           raw_lead=raw_lead)
    _check(nice, outs, poison, imgs, WINDOWS, (6, 8), FLIPS, consts, "float16", 8, 6)


@pytest.mark.parametrize("dt,layout", [(F16, PLANAR), (F32, INTERLEAVED)])
@pytest.mark.parametrize("size", [(12, 16), (6, 8), (9, 23)])
def test_resize_skips_elements_of_failed_and_unreadable_slots(nice, ctx, size, dt, layout):
    """A slot with a nonzero status and a slot with nothing to read: exactly the
    elements with a tap in one of them keep the poison, also where the window
    has the output's size (an element then depends on one slot)."""
    imgs = _images()
    consts = const_sets(nice)["unit"]
    windows = [(0, 6, 4, 8, 6), (0, 9, 7, 20, 12), (0, 4, 4, 16, 12), (1, 30, 22, 7, 7)]
    flips = [0, 1, 0, 1]
    # positions: window 0 has 4 slots (0..3), window 1 9 (4..12), window 2 9 (13..21), window 3 4 (22..25)
    counts = [len(_touched(SHAPES[i][0], SHAPES[i][1], 8, 6, x0, y0, rw, rh)) for i, x0, y0, rw, rh in windows]
    assert counts == [4, 9, 9, 4]
    failed = {1, 8, 13}
    none = {10, 21}
    kinds = [KIND_NONE if p in none else (KIND_RAW if p % 4 == 2 else KIND_DENSE) for p in range(sum(counts))]
    bad, p = {}, 0
    for j, (i, x0, y0, rw, rh) in enumerate(windows):
        for ti in _touched(SHAPES[i][0], SHAPES[i][1], 8, 6, x0, y0, rw, rh):
            if p in failed or p in none:
                bad.setdefault(j, []).append(ti)
            p += 1
    assert sorted(bad) == [0, 1, 2]
    outs, poison = _resize(nice, ctx, imgs, 8, 6, windows, size, dt, layout, [0, 4, 0, 1], flips, consts, kinds=kinds,
                           failed=failed)
    _check(nice, outs, poison, imgs, windows, size, flips, consts, DTYPES[dt], 8, 6, bad=bad)
    for j in bad:                                          # and the test sees both: kept and written elements
        assert (outs[j] == poison).any() and (outs[j] != poison).any(), j


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("dt", [F32, F16, BF16])
def test_identity_size_equals_the_tensor_merge(nice, ctx, dt, layout):
    """Windows of the output's size: nice_set_merge_tensor_dev's bits on the same slots."""
    imgs = [np.concatenate([im, _random_image(im.shape[1], im.shape[0], 1, 5)], axis=2) for im in _images()]
    windows = [(0, 3, 2, 10, 7), (0, 30, 23, 10, 7), (1, 27, 0, 10, 7), (1, 0, 22, 10, 7)]
    leads, flips = [0, 1, 2, 4], [0, 1, 1, 0]
    consts = const_sets(nice)["odd"]
    got, _ = _resize(nice, ctx, imgs, 8, 6, windows, (7, 10), dt, layout, leads, flips, consts)
    want, _ = _merge_tensor(nice, ctx, imgs, 8, 6, windows, dt, layout, leads, flips, "odd")
    for wdw, a, b in zip(windows, got, want):
        assert np.array_equal(a, b), wdw


def check_float16_rounds_twice(nice, ctx, run, layout):
    """float16 on the constants whose elements differ between one rounding and
    two (tests/test_sets_tensor_cpu.py), through `run` (_resize, or the
    antialiased harness): three windows of the output's size, so acc = b << 16
    and an element is the table's; each holds the 14 entries, planted; stores of
    4, 1 and 2 elements, one window mirrored."""
    imgs = _images()
    windows = [(0, 3, 2, 10, 7), (0, 30, 23, 10, 7), (1, 27, 0, 10, 7)]
    leads, flips = [0, 1, 2], [0, 1, 0]
    for i, x0, y0, rw, rh in windows:
        plant_halfway(imgs[i], x0, y0, rw, rh)
        assert holds_halfway(imgs[i][y0:y0 + rh, x0:x0 + rw])
    table = lut_bits(nice, "halfway", "float16")
    got, _ = run(nice, ctx, imgs, 8, 6, windows, (7, 10), F16, layout, leads, flips, const_sets(nice)["halfway"])
    for (i, x0, y0, rw, rh), flip, a in zip(windows, flips, got):
        assert np.array_equal(a, expect_bits(table, imgs[i][y0:y0 + rh, x0:x0 + rw], flip)), (i, x0, y0)


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
def test_identity_size_float16_rounds_twice(nice, ctx, layout):
    check_float16_rounds_twice(nice, ctx, _resize, layout)


# ---- 2. end to end on the reference set -------------------------------------------------------------
# windows of different sizes and aspects: inside the raw tile, across four tiles with the raw one among them, image
# edges, a whole image, a one-row image
RCROPS = [(0, 70, 70, 48, 40), (0, 40, 40, 60, 75), (0, 120, 60, 80, 76), (1, 100, 100, 33, 57), (1, 250, 150, 83, 61),
          (4, 0, 0, 64, 64), (5, 82, 30, 20, 17), (2, 10, 0, 40, 1), (3, 0, 0, 5, 7)]
RFLIPS = [1, 0, 1, 0, 0, 1, 0, 1, 1]
RSIZE = (24, 32)


def _want_batch(r, windows, size, flips, consts, dtype):
    return np.stack([model_bits(r.imgs[i][y0:y0 + rh, x0:x0 + rw], size[0], size[1], f, consts[0], consts[1], dtype)
                     for (i, x0, y0, rw, rh), f in zip(windows, flips)])


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("c", [3, 4])
def test_resized_crop_batch(nice, O, ctx, c, channels_last):
    import torch
    r = ref(O, c)
    iset = encoded(nice, O, ctx, c)
    consts = nice.normalize_affine((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    out = nice.decode_set_resized(iset, windows=RCROPS, size=RSIZE, scale=consts[0], bias=consts[1], flip=RFLIPS,
                                  channels_last=channels_last, ctx=ctx)
    assert tuple(out.shape) == (len(RCROPS), 3) + RSIZE and out.dtype == torch.float16
    assert out.stride(1) == 1 and out.stride(3) == 3 if channels_last else out.is_contiguous()
    assert last_set(nice, ctx) == _slot_counts(r, RCROPS) and last_set(nice, ctx)[1] >= 2   # the raw tile, in several windows
    assert np.array_equal(bits_of(torch, out), _want_batch(r, RCROPS, RSIZE, RFLIPS, consts, "float16"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_size_equals_decode_set_tensor(nice, O, ctx, dtype):
    import torch
    iset = encoded(nice, O, ctx, 4)
    scale, bias = const_sets(nice)["imagenet"]
    td = _tdtype(torch, dtype)
    want = nice.decode_set_tensor(iset, windows=CROPS, dtype=td, scale=scale, bias=bias, flip=CROP_FLIPS, ctx=ctx)
    got = nice.decode_set_resized(iset, windows=CROPS, size=(40, 48), dtype=td, scale=scale, bias=bias, flip=CROP_FLIPS,
                                  ctx=ctx)
    assert np.array_equal(bits_of(torch, got), np.stack([bits_of(torch, w) for w in want]))


def test_resized_into_strided_views(nice, O, ctx):
    """Views of poisoned larger tensors, planar and channels_last, and a list of views: nothing outside changes."""
    import torch
    r = ref(O, 4)
    iset = encoded(nice, O, ctx, 4)
    consts = const_sets(nice)["imagenet"]
    want = _want_batch(r, RCROPS, RSIZE, RFLIPS, consts, "bfloat16")
    m, (oh, ow) = len(RCROPS), RSIZE
    planar = torch.full((m, 4, oh + 3, ow + 5), POISON, dtype=torch.bfloat16, device="cuda")
    nhwc = torch.full((m, oh + 3, ow + 5, 3), POISON, dtype=torch.bfloat16, device="cuda")
    for big, view in ((planar, planar[:, 1:, 2:-1, 3:-2]), (nhwc, nhwc.permute(0, 3, 1, 2)[:, :, 2:-1, 3:-2])):
        assert tuple(view.shape) == (m, 3, oh, ow)
        assert nice.decode_set_resized(iset, windows=RCROPS, size=RSIZE, out=view, dtype=torch.bfloat16, scale=consts[0],
                                       bias=consts[1], flip=RFLIPS, ctx=ctx) is view
        assert np.array_equal(bits_of(torch, view), want)
        view.fill_(POISON)
        assert bool((big == POISON).all())
    bigs = [torch.full((3, oh + 2, ow + 5), POISON, dtype=torch.bfloat16, device="cuda") for _ in RCROPS]
    views = [b[:, 1:-1, 3:-2] for b in bigs]
    back = nice.decode_set_resized(iset, windows=RCROPS, size=RSIZE, out=views, dtype=torch.bfloat16, scale=consts[0],
                                   bias=consts[1], flip=RFLIPS, ctx=ctx)
    assert all(a is b for a, b in zip(back, views))
    for j, (big, view) in enumerate(zip(bigs, views)):
        assert np.array_equal(bits_of(torch, view), want[j]), j
        view.fill_(POISON)
        assert bool((big == POISON).all())


def test_damaged_tile_leaves_its_elements(nice, O, ctx):
    """The corruption of tests/test_sets_tensor.py: one coded tile of image 1
    fails, in every window that touches it; the elements with a tap in it keep
    the poison, the others are right."""
    import torch
    r = ref(O, 4)
    iset = encoded(nice, O, ctx, 4)
    bad_ti = 7                                             # tile (1, 1) of image 1's 6 x 4 grid
    bad_t = r.first[1] + bad_ti
    assert r.kind[bad_t] == 0
    packed = iset.packed.clone()
    packed[int(iset.off[bad_t]) + 13 + 3] ^= 0xFF          # inside the table header, which follows the 13-byte file header
    hurt = dataclasses.replace(iset, packed=packed)
    consts = const_sets(nice)["unit"]
    poison = int(bits_of(torch, torch.tensor([POISON], dtype=torch.float16))[0])
    windows = [(1, 60, 60, 10, 10), (1, 70, 70, 20, 20), (1, 130, 70, 20, 20), (1, 50, 100, 30, 40)]
    flips = [1, 0, 1, 0]
    size = (13, 16)
    out = torch.full((4, 3) + size, POISON, dtype=torch.float16, device="cuda")
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set_resized(hurt, windows=windows, size=size, out=out, flip=flips, ctx=ctx)
    st = e.value.statuses
    assert len(st) == 10 and [s < 0 for s in st] == [False, False, False, True, True, False] + [False, True, False, False]
    assert e.value.out is out
    got = bits_of(torch, out)
    for j, wdw in enumerate(windows):
        want = expect_window(r.imgs[1], wdw, size, flips[j], consts, "float16", 64, 64, poison, bad_tiles=[bad_ti])
        assert np.array_equal(got[j], want), wdw
    assert (got[0] == poison).any() and (got[0] != poison).any()
    assert (got[1] == poison).all() and (got[2] != poison).all()


def _merges(nice, ctx):
    L = nice.lib()
    L.nice_test_last_set_merges.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    n = ctypes.c_uint32()
    assert L.nice_test_last_set_merges(ctx.ptr, ctypes.byref(n)) == 0
    return n.value


def test_launch_counts(nice, O):
    """The batch decode's launches are decode_set_tensor's, whatever M is (the
    phase counters of tests/test_sets_tensor.py, which see the decode and not
    the merges); the merges are one launch where decode_set_tensor makes two
    for a set with coded and raw tiles (the library's own count)."""
    import torch
    ctx = nice.Context(0)
    imgs = _cuda(torch, ref(O, 4).imgs)
    six = nice.encode_set(imgs, tile=(64, 64), ctx=ctx)
    small = [(i, 0, 0, 5, 1) for i in range(K)] * 3
    L = nice.lib()
    L.nice_ctx_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.nice_ctx_set_timing(ctx.ptr, 1) == 0
    try:
        _timing(nice, ctx)
        nice.decode_set_tensor(six, ctx=ctx)
        tensor = _timing(nice, ctx)
        assert _merges(nice, ctx) == 2 and last_set(nice, ctx) == (45, 1)
        counts = []
        for kw in (dict(images=[0]), dict(), dict(windows=small), dict(windows=RCROPS)):
            nice.decode_set_resized(six, size=(8, 8), ctx=ctx, **kw)
            counts.append(_timing(nice, ctx))
            assert _merges(nice, ctx) == 1, kw
        assert tensor[PH_DEC_TABLES] > 0
        for c in counts:
            assert c[PH_DEC_TABLES] == tensor[PH_DEC_TABLES]
    finally:
        L.nice_ctx_set_timing(ctx.ptr, 0)


# ---- 3. host refusals ---------------------------------------------------------------------------------
def test_rejects(nice, O, ctx):
    import torch
    iset = encoded(nice, O, ctx, 3)
    two = [(0, 0, 0, 48, 40), (1, 0, 0, 30, 20)]

    def bad(**kw):
        kw.setdefault("size", (8, 12))
        with pytest.raises(nice.NiceError) as e:
            nice.decode_set_resized(iset, ctx=ctx, **kw)
        assert e.value.code == E_ARG, kw

    def empty(*shape, dtype=torch.float16, device="cuda"):
        return torch.empty(shape, dtype=dtype, device=device)

    for size in ((0, 8), (8, 0), (8193, 8), (8, 8193), (8,), None, (8, 8, 8)):
        bad(windows=two, size=size)
    bad(dtype=torch.float64)
    for shape in ((2, 3, 12, 8), (3, 3, 8, 12), (2, 8, 12, 3), (2, 4, 8, 12), (2, 3, 8)):
        bad(windows=two, out=empty(*shape))
    bad(windows=two, out=[empty(3, 8, 12)])
    bad(windows=two, out=empty(2, 3, 8, 12, device="cpu"))
    bad(windows=two, out=empty(2, 3, 8, 12, dtype=torch.float32))                   # not the dtype asked for
    bad(windows=two, out=empty(2, 3, 8, 24)[:, :, :, ::2])                          # innermost stride 2: neither layout
    bad(windows=two, out=[empty(3, 8, 12), empty(8, 12, 3).permute(2, 0, 1)])       # two layouts in one call
    bad(windows=two, out=empty(2 * 3 * 8 * 12).as_strided((2, 3, 8, 12), (288, 96, 11, 1)))        # row pitch < ow
    bad(windows=two, flip=[1])
    bad(scale=(float("inf"), 1, 1))
    bad(images=[0], windows=two)
    bad(windows=[(0, 150, 100, 51, 1)])
    bad(flags=nice.DEC_STRICT_REFERENCE)
    # the C entry point
    L = nice.lib()
    out = empty(2, 3, 8, 12)
    st = torch.zeros(64, dtype=torch.int32, device="cuda")
    off, lens, kind = iset.off.contiguous(), iset.stream_len.contiguous(), iset.kind.contiguous()
    n = iset.first[-1]
    one = (ctypes.c_float * 3)(1, 1, 1)

    def call(dt=F16, layout=PLANAR, ow=12, oh=8, base=0, flags=0, pitch=12):
        return L.nice_decode_set_resized_dev(
            ctx.ptr, None, ctypes.c_void_p(iset.packed.data_ptr()), int(off[n]), ctypes.c_void_p(off.data_ptr()),
            ctypes.c_void_p(lens.data_ptr()), ctypes.c_void_p(kind.data_ptr()),
            (ctypes.c_uint32 * K)(*iset.widths), (ctypes.c_uint32 * K)(*iset.heights), K, 64, 64,
            (ctypes.c_uint32 * 10)(*[v for w in two for v in w]), None, ow, oh,
            (ctypes.c_void_p * 2)(out[0].data_ptr() + base, out[1].data_ptr() + base),
            (ctypes.c_uint64 * 2)(pitch, pitch), (ctypes.c_uint64 * 2)(96, 96), 2, dt, layout, one, one, flags,
            ctypes.c_void_p(st.data_ptr()))

    assert call(ow=0) == E_ARG and call(oh=0) == E_ARG and call(ow=8193) == E_ARG and call(oh=8193) == E_ARG
    assert call(dt=3) == E_ARG and call(layout=2) == E_ARG and call(base=1) == E_ARG
    assert call(flags=nice.DEC_STRICT_REFERENCE) == E_ARG
    assert call(pitch=11) == E_ARG and call(layout=INTERLEAVED) == E_ARG            # row pitch 12 < 3 * 12
    assert call() == 0
    torch.cuda.synchronize()
