"""Image sets, antialiased resized tensor output (include/nice.h, "image sets:
antialiased resized tensor output") on the GPU: the two kernels alone on random
bytes in hand-built slots, then decode_set_resized(antialias=True) end to end
on the reference set of tests/test_sets.py, then the host refusals.

The reference is the numpy model of tests/test_sets_resize_aa_cpu.py (weights
in Python integers, h and acc32 in int64, the element as the single rounding of
the exact rational).  Every comparison is bit for bit on the integer view;
poisoned guards surround every output, and an element whose tap rectangle meets
a failed or unreadable slot must keep the poison."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_sets import (CROPS, K, PH_DEC_TABLES, _cuda, _random_image, _slot_counts, _timing, _touched, encoded, last_set,
                       ref)
from test_sets_tensor import (BF16, CROP_FLIPS, DTYPES, F16, F32, INTERLEAVED, PLANAR, POISON, POISON_BITS, _merge_tensor,
                              _tdtype, bits_of)
from test_sets_tensor_cpu import const_sets
from test_sets_resize import (FLIPS, KIND_DENSE, KIND_NONE, KIND_RAW, LEADS, ODD, RCROPS, RFLIPS, RSIZE, SHAPES, SIZES,
                              WINDOWS, _images, _merges, _resize, check_float16_rounds_twice, garbage_tiles)
from test_sets_resize_cpu import model_bits
from test_sets_resize_aa_cpu import aa_taps, model_bits_aa, tap_ranges

pytestmark = pytest.mark.gpu

E_ARG = -1
AA = "nice_set_resize_aa_tensor_dev"


@pytest.fixture(scope="module")
def ctx(nice):
    return nice.Context(0)


def rect_tiles_hit(wdw, size, flip, tw, th, nx, bad_tiles):
    """[oh, ow] bool: the elements whose tap rectangle (the model's tap ranges) meets one of bad_tiles."""
    _, x0, y0, rw, rh = wdw
    oh, ow = size
    clo, chi = tap_ranges(rw, ow, bool(flip))
    rlo, rhi = tap_ranges(rh, oh)
    hit = np.zeros((oh, ow), bool)
    for ti in bad_tiles:
        ty, tx = divmod(ti, nx)
        cols = ((x0 + clo) // tw <= tx) & (tx <= (x0 + chi) // tw)
        rows = ((y0 + rlo) // th <= ty) & (ty <= (y0 + rhi) // th)
        hit |= rows[:, None] & cols[None, :]
    return hit


def expect_window(img, wdw, size, flip, consts, dtype, tw, th, poison, bad_tiles=()):
    _, x0, y0, rw, rh = wdw
    want = model_bits_aa(img[y0:y0 + rh, x0:x0 + rw], size[0], size[1], bool(flip), consts[0], consts[1], dtype).copy()
    if bad_tiles:
        want[:, rect_tiles_hit(wdw, size, flip, tw, th, -(-img.shape[1] // tw), bad_tiles)] = poison
    return want


# ---- 1. the kernels alone ---------------------------------------------------------------------
def _resize_aa(nice, ctx, imgs, tw, th, windows, size, dt, layout, leads, flips, consts, kinds=None, raw_lead=0,
               failed=(), odd_pitch=(), no_status=False):
    """tests/test_sets_resize.py's _resize, through nice_set_resize_aa_tensor_dev: the same slots (dense with
    noise in byte +3, raw at raw_lead bytes past a multiple of 16, or none), statuses, poisoned and guarded
    outputs.  Returns each window's bits [3, oh, ow] and the poison."""
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
        shift = 8 + lead + (7 if j in odd_pitch else 0)
        row = (n_el + 7) // 8 * 8 + 24 + (1 if j in odd_pitch else 0)
        rows = oh + 3                                        # a guard row above, two below (between planes)
        big = torch.full((3 if layout == PLANAR else 1, rows, row), poison, dtype=idt, device="cuda")
        assert big.data_ptr() % 16 == 0
        bigs.append(big)
        ptrs.append(big.data_ptr() + (row + shift) * es)
        rps.append(row)
        pps.append(rows * row)
        where.append((slice(1, 1 + oh), slice(shift, shift + n_el)))
    scale, bias = consts
    m = len(windows)
    rc = getattr(nice.lib(), AA)(
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


def _check(outs, poison, imgs, windows, size, flips, consts, dtype, tw, th, bad=None):
    for j, (wdw, got) in enumerate(zip(windows, outs)):
        want = expect_window(imgs[wdw[0]], wdw, size, flips[j], consts, dtype, tw, th, poison,
                             () if bad is None else bad.get(j, ()))
        assert np.array_equal(got, want), (j, wdw, size)


def test_the_sizes_cover_every_kind_of_window():
    """On one launch: enlarging windows, reducing ones, the 37 x 29 window to one element (37 and 29 taps),
    windows that reduce on one axis only."""
    kinds = set()
    for oh, ow in SIZES:
        for _, _, _, rw, rh in WINDOWS:
            kinds.add((ow < rw, oh < rh))
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    assert (1, 1) in SIZES and (37, 29) in [(rw, rh) for _, _, _, rw, rh in WINDOWS]
    assert len(aa_taps(37, 1)[0][1]) == 37 and len(aa_taps(29, 1)[0][1]) == 29
    assert {(ow < rw, oh < rh) for oh, ow in SIZES[:2] for _, _, _, rw, rh in WINDOWS} >= {(True, False), (False, True)}


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("dt", [F32, F16, BF16])
@pytest.mark.parametrize("size", SIZES)
def test_resize_aa_matches_model(nice, ctx, size, dt, layout):
    imgs = _images()
    consts = const_sets(nice)["imagenet"]
    outs, poison = _resize_aa(nice, ctx, imgs, 8, 6, WINDOWS, size, dt, layout, LEADS, FLIPS, consts, odd_pitch=ODD)
    _check(outs, poison, imgs, WINDOWS, size, FLIPS, consts, DTYPES[dt], 8, 6)


@pytest.mark.parametrize("dt,layout,size", [(F16, PLANAR, (12, 16)), (F32, INTERLEAVED, (7, 70)), (BF16, PLANAR, (33, 5))])
def test_resize_aa_other_tile_size(nice, ctx, dt, layout, size):
    """Tiles of 16 x 8, no status column, the other constants."""
    imgs = _images()
    consts = const_sets(nice)["odd"]
    flips = [1 - f for f in FLIPS]
    outs, poison = _resize_aa(nice, ctx, imgs, 16, 8, WINDOWS, size, dt, layout, LEADS, flips, consts, no_status=True)
    _check(outs, poison, imgs, WINDOWS, size, flips, consts, DTYPES[dt], 16, 8)


def _kernel_constants():
    text = open(os.path.join(ROOT, "fast-losless-image-compression-format_amd", "csrc", "nice_sets_resize_aa.hip")).read()
    lds = int(re.search(r"constexpr uint32_t AA_LDS_PX = (\d+);", text).group(1))
    rows = int(re.search(r"constexpr uint32_t AA_ROWS = (\d+);", text).group(1))
    assert re.search(r"constexpr uint32_t AA_COLS = TL_THREADS;", text)
    return lds, rows


def _long_cases():
    """(image w, h), size, flip.  A 515 x 130 image to 7 x 9 (115 column taps, more than a wave, and 37 row
    taps) and to 3 x 300 (an output row longer than a block's 256 columns, 87 row taps).  And from the
    kernel's constants: a block stages at most AA_LDS_PX source columns at a time and no loop over taps is
    unrolled or vectorised, so the smallest window that leaves one stage is AA_LDS_PX + 1 pixels wide under
    one block of columns; its rows, 2 AA_ROWS + 1 to AA_ROWS + 1, take two bands."""
    lds, rows = _kernel_constants()
    return [((515, 130), (7, 9), 1), ((515, 130), (3, 300), 0), ((lds + 1, 2 * rows + 1), (rows + 1, 3), 1)]


@pytest.mark.parametrize("case", [0, 1, 2])
@pytest.mark.parametrize("dt,layout", [(F32, PLANAR), (F16, INTERLEAVED)])
def test_long_tap_runs(nice, ctx, case, dt, layout):
    (w, h), size, flip = _long_cases()[case]
    img = _random_image(w, h, 3, 40 + case)
    consts = const_sets(nice)["imagenet"]
    windows = [(0, 0, 0, w, h)]
    if case == 0:
        assert max(len(t) for _, t in aa_taps(515, 9)) > 64 and max(len(t) for _, t in aa_taps(130, 7)) >= 37
    if case == 2:
        assert len(aa_taps(w, 3)[1][1]) > 1000
    outs, poison = _resize_aa(nice, ctx, [img], 16, 8, windows, size, dt, layout, [1], [flip], consts)
    _check(outs, poison, [img], windows, size, [flip], consts, DTYPES[dt], 16, 8)


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("raw_lead", [0, 1, 5])
def test_resize_aa_raw_and_dense_slots_mixed(nice, ctx, raw_lead, layout):
    imgs = _images()
    consts = const_sets(nice)["imagenet"]
    ns = sum(len(_touched(SHAPES[i][0], SHAPES[i][1], 8, 6, x0, y0, rw, rh)) for i, x0, y0, rw, rh in WINDOWS)
    kinds = [KIND_RAW if p % 3 == 1 else KIND_DENSE for p in range(ns)]
    assert set(kinds[1:5]) == {KIND_DENSE, KIND_RAW}                     # the 2 x 2 window (positions 1..4) mixes
    for size in ((6, 8), (9, 23)):
        outs, poison = _resize_aa(nice, ctx, imgs, 8, 6, WINDOWS, size, BF16, layout, LEADS, FLIPS, consts, kinds=kinds,
                                  raw_lead=raw_lead)
        _check(outs, poison, imgs, WINDOWS, size, FLIPS, consts, "bfloat16", 8, 6)
    kinds = [KIND_RAW] * ns
    outs, poison = _resize_aa(nice, ctx, imgs, 8, 6, WINDOWS, (5, 1), F16, layout, LEADS, FLIPS, consts, kinds=kinds,
                              raw_lead=raw_lead)
    _check(outs, poison, imgs, WINDOWS, (5, 1), FLIPS, consts, "float16", 8, 6)


@pytest.mark.parametrize("dt,layout", [(F16, PLANAR), (F32, INTERLEAVED)])
@pytest.mark.parametrize("size", [(12, 16), (6, 8), (9, 23)])
def test_resize_aa_skips_elements_of_failed_and_unreadable_slots(nice, ctx, size, dt, layout):
    """A slot with a nonzero status and a slot with nothing to read: exactly the elements whose tap rectangle
    (the model's tap ranges, not two taps) meets one of them keep the poison."""
    imgs = _images()
    consts = const_sets(nice)["unit"]
    windows = [(0, 6, 4, 8, 6), (0, 9, 7, 20, 12), (0, 4, 4, 16, 12), (1, 30, 22, 7, 7)]
    flips = [0, 1, 0, 1]
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
    outs, poison = _resize_aa(nice, ctx, imgs, 8, 6, windows, size, dt, layout, [0, 4, 0, 1], flips, consts, kinds=kinds,
                              failed=failed)
    _check(outs, poison, imgs, windows, size, flips, consts, DTYPES[dt], 8, 6, bad=bad)
    for j in bad:                                          # and the test sees both: kept and written elements
        assert (outs[j] == poison).any() and (outs[j] != poison).any(), j


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("dt", [F32, F16, BF16])
def test_non_reducing_windows_equal_the_plain_resize(nice, ctx, dt, layout):
    """Windows that reduce on neither axis: nice_set_resize_tensor_dev's bits on the same slots."""
    imgs = _images()
    consts = const_sets(nice)["imagenet"]
    size = (12, 20)
    keep = [j for j, w in enumerate(WINDOWS) if w[3] <= size[1] and w[4] <= size[0]]
    assert len(keep) >= 7
    windows, leads, flips = [WINDOWS[j] for j in keep], [LEADS[j] for j in keep], [FLIPS[j] for j in keep]
    got, _ = _resize_aa(nice, ctx, imgs, 8, 6, windows, size, dt, layout, leads, flips, consts)
    want, _ = _resize(nice, ctx, imgs, 8, 6, windows, size, dt, layout, leads, flips, consts)
    for wdw, a, b in zip(windows, got, want):
        assert np.array_equal(a, b), wdw


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("dt", [F32, F16, BF16])
def test_identity_size_equals_the_tensor_merge(nice, ctx, dt, layout):
    imgs = [np.concatenate([im, _random_image(im.shape[1], im.shape[0], 1, 5)], axis=2) for im in _images()]
    windows = [(0, 3, 2, 10, 7), (0, 30, 23, 10, 7), (1, 27, 0, 10, 7), (1, 0, 22, 10, 7)]
    leads, flips = [0, 1, 2, 4], [0, 1, 1, 0]
    consts = const_sets(nice)["odd"]
    got, _ = _resize_aa(nice, ctx, imgs, 8, 6, windows, (7, 10), dt, layout, leads, flips, consts)
    want, _ = _merge_tensor(nice, ctx, imgs, 8, 6, windows, dt, layout, leads, flips, "odd")
    for wdw, a, b in zip(windows, got, want):
        assert np.array_equal(a, b), wdw


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
def test_identity_size_float16_rounds_twice(nice, ctx, layout):
    """The filter's elements too are the float32 fmaf rounded again (tests/test_sets_resize.py)."""
    check_float16_rounds_twice(nice, ctx, _resize_aa, layout)


# ---- 2. end to end on the reference set -------------------------------------------------------------
def _want_batch(r, windows, size, flips, consts, dtype, model=model_bits_aa):
    return np.stack([model(r.imgs[i][y0:y0 + rh, x0:x0 + rw], size[0], size[1], bool(f), consts[0], consts[1], dtype)
                     for (i, x0, y0, rw, rh), f in zip(windows, flips)])


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("c", [3, 4])
def test_resized_crop_batch_antialiased(nice, O, ctx, c, channels_last):
    import torch
    r = ref(O, c)
    iset = encoded(nice, O, ctx, c)
    # (the filtered gradients of the reference set cross zero under a mean-and-std normalisation, and the
    # model covers values that are normal in all three types: those constants are with the kernels alone)
    consts = const_sets(nice)["odd"]
    out = nice.decode_set_resized(iset, windows=RCROPS, size=RSIZE, scale=consts[0], bias=consts[1], flip=RFLIPS,
                                  channels_last=channels_last, ctx=ctx, antialias=True)
    assert tuple(out.shape) == (len(RCROPS), 3) + RSIZE and out.dtype == torch.float16
    assert out.stride(1) == 1 and out.stride(3) == 3 if channels_last else out.is_contiguous()
    assert last_set(nice, ctx) == _slot_counts(r, RCROPS) and last_set(nice, ctx)[1] >= 2
    assert np.array_equal(bits_of(torch, out), _want_batch(r, RCROPS, RSIZE, RFLIPS, consts, "float16"))
    # antialias=False in the same session: still the sampled value
    plain = nice.decode_set_resized(iset, windows=RCROPS, size=RSIZE, scale=consts[0], bias=consts[1], flip=RFLIPS,
                                    channels_last=channels_last, ctx=ctx, antialias=False)
    want = _want_batch(r, RCROPS, RSIZE, RFLIPS, consts, "float16", model=model_bits)
    assert np.array_equal(bits_of(torch, plain), want)
    assert not np.array_equal(bits_of(torch, plain), bits_of(torch, out))


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_size_equals_decode_set_tensor(nice, O, ctx, dtype):
    import torch
    iset = encoded(nice, O, ctx, 4)
    scale, bias = const_sets(nice)["imagenet"]
    td = _tdtype(torch, dtype)
    want = nice.decode_set_tensor(iset, windows=CROPS, dtype=td, scale=scale, bias=bias, flip=CROP_FLIPS, ctx=ctx)
    got = nice.decode_set_resized(iset, windows=CROPS, size=(40, 48), dtype=td, scale=scale, bias=bias, flip=CROP_FLIPS,
                                  ctx=ctx, antialias=True)
    assert np.array_equal(bits_of(torch, got), np.stack([bits_of(torch, w) for w in want]))


def test_resized_into_strided_views(nice, O, ctx):
    """Views of poisoned larger tensors, planar and channels_last, and a list of views: nothing outside changes."""
    import torch
    r = ref(O, 4)
    iset = encoded(nice, O, ctx, 4)
    consts = const_sets(nice)["odd"]
    want = _want_batch(r, RCROPS, RSIZE, RFLIPS, consts, "bfloat16")
    m, (oh, ow) = len(RCROPS), RSIZE
    kw = dict(windows=RCROPS, size=RSIZE, dtype=torch.bfloat16, scale=consts[0], bias=consts[1], flip=RFLIPS, ctx=ctx,
              antialias=True)
    planar = torch.full((m, 4, oh + 3, ow + 5), POISON, dtype=torch.bfloat16, device="cuda")
    nhwc = torch.full((m, oh + 3, ow + 5, 3), POISON, dtype=torch.bfloat16, device="cuda")
    for big, view in ((planar, planar[:, 1:, 2:-1, 3:-2]), (nhwc, nhwc.permute(0, 3, 1, 2)[:, :, 2:-1, 3:-2])):
        assert tuple(view.shape) == (m, 3, oh, ow)
        assert nice.decode_set_resized(iset, out=view, **kw) is view
        assert np.array_equal(bits_of(torch, view), want)
        view.fill_(POISON)
        assert bool((big == POISON).all())
    bigs = [torch.full((3, oh + 2, ow + 5), POISON, dtype=torch.bfloat16, device="cuda") for _ in RCROPS]
    views = [b[:, 1:-1, 3:-2] for b in bigs]
    back = nice.decode_set_resized(iset, out=views, **kw)
    assert all(a is b for a, b in zip(back, views))
    for j, (big, view) in enumerate(zip(bigs, views)):
        assert np.array_equal(bits_of(torch, view), want[j]), j
        view.fill_(POISON)
        assert bool((big == POISON).all())


def test_damaged_tile_leaves_its_elements(nice, O, ctx):
    """The damaged tile of tests/test_sets_resize.py, with the rectangle rule."""
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
        nice.decode_set_resized(hurt, windows=windows, size=size, out=out, flip=flips, ctx=ctx, antialias=True)
    st = e.value.statuses
    assert len(st) == 10 and [s < 0 for s in st] == [False, False, False, True, True, False] + [False, True, False, False]
    assert e.value.out is out
    got = bits_of(torch, out)
    for j, wdw in enumerate(windows):
        want = expect_window(r.imgs[1], wdw, size, flips[j], consts, "float16", 64, 64, poison, bad_tiles=[bad_ti])
        assert np.array_equal(got[j], want), wdw
    assert (got[0] == poison).any() and (got[0] != poison).any()
    assert (got[1] == poison).all() and (got[2] != poison).all()
    assert (got[3] == poison).any() and (got[3] != poison).any()


def test_launch_counts(nice, O):
    """The batch decode's launches are decode_set_tensor's whatever M is; the resample launches are two (the
    weight tables, the filter) whatever the windows are."""
    import torch
    ctx = nice.Context(0)
    imgs = _cuda(torch, ref(O, 4).imgs)
    six = nice.encode_set(imgs, tile=(64, 64), ctx=ctx)
    small = [(i, 0, 0, 5, 1) for i in range(K)] * 3
    assert len(small) == 18
    L = nice.lib()
    L.nice_ctx_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.nice_ctx_set_timing(ctx.ptr, 1) == 0
    try:
        _timing(nice, ctx)
        nice.decode_set_tensor(six, ctx=ctx)
        tensor = _timing(nice, ctx)
        counts, merges = [], []
        for kw in (dict(images=[0]), dict(), dict(windows=small), dict(windows=RCROPS)):
            nice.decode_set_resized(six, size=(8, 8), ctx=ctx, antialias=True, **kw)
            counts.append(_timing(nice, ctx))
            merges.append(_merges(nice, ctx))
        assert merges == [2, 2, 2, 2]
        assert tensor[PH_DEC_TABLES] > 0
        for c in counts:
            assert c[PH_DEC_TABLES] == tensor[PH_DEC_TABLES]
        nice.decode_set_resized(six, size=(8, 8), ctx=ctx)
        assert _merges(nice, ctx) == 1                       # the sampled call keeps its one launch
    finally:
        L.nice_ctx_set_timing(ctx.ptr, 0)


# ---- 3. host refusals ---------------------------------------------------------------------------------
def test_rejects(nice, O, ctx):
    """The sibling's refusals, through the Python call and the C entry point.  (The limit of 65536 pixels on a
    reducing axis is tested on the CPU: no call here claims an image that large.)"""
    import torch
    iset = encoded(nice, O, ctx, 3)
    two = [(0, 0, 0, 48, 40), (1, 0, 0, 30, 20)]

    def bad(**kw):
        kw.setdefault("size", (8, 12))
        with pytest.raises(nice.NiceError) as e:
            nice.decode_set_resized(iset, ctx=ctx, antialias=True, **kw)
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
    bad(windows=two, out=empty(2, 3, 8, 12, dtype=torch.float32))
    bad(windows=two, out=empty(2, 3, 8, 24)[:, :, :, ::2])
    bad(windows=two, out=[empty(3, 8, 12), empty(8, 12, 3).permute(2, 0, 1)])
    bad(windows=two, out=empty(2 * 3 * 8 * 12).as_strided((2, 3, 8, 12), (288, 96, 11, 1)))
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
        return L.nice_decode_set_resized_aa_dev(
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
