"""Image sets decoded straight into normalised float tensors (include/nice.h,
"image sets: tensor output"): the tensor merge kernel alone on random bytes,
then decode_set_tensor end to end on the reference set of tests/test_sets.py.

The reference is a table: element = fmaf(b, scale[c], bias[c]) in float32 is,
for the constant sets used here, the double b * scale + bias rounded once
(tests/test_sets_tensor_cpu.py asserts that with rationals), and torch's CPU
conversion to float16 / bfloat16 rounds to nearest even.  Every comparison is
bit for bit, on the integer view; no entry is subnormal or infinite."""
import ctypes
import dataclasses

import numpy as np
import pytest

from test_tiled import np_tiles
from test_sets import (CROPS, K, MERGE_SHAPES, MERGE_WINDOWS, PH_DEC_TABLES, PH_ENC_CLASSIFY, _cuda, _random_image,
                       _slot_counts, _timing, _touched, encoded, last_set, ref)
from test_sets_tensor_cpu import HALFWAY, const_sets, lut32

pytestmark = pytest.mark.gpu

E_ARG = -1
F32, F16, BF16 = 0, 1, 2
PLANAR, INTERLEAVED = 0, 1
DTYPES = ["float32", "float16", "bfloat16"]
POISON_BITS = {4: 0x7E7E7E7E, 2: 0x7E7E}          # float16: a NaN; float32 and bfloat16: beyond any entry of the tables
POISON = -768.0                                   # the same idea for torch tensors: exact in all three types
CROP_FLIPS = [1, 0, 1, 0, 0, 1, 0, 1]


@pytest.fixture(scope="module")
def ctx(nice):
    return nice.Context(0)


def _tdtype(torch, name):
    return getattr(torch, name)


_LUT = {}


def lut_bits(nice, consts, dtype):
    """[256, 3] integers: the bits of the expected element for every byte and
    channel (built once per constant set and type, on the CPU)."""
    import torch
    if (consts, dtype) not in _LUT:
        scale, bias = const_sets(nice)[consts]
        t32 = lut32(scale, bias)
        mag = np.abs(t32.astype(np.float64))
        assert np.isfinite(t32).all() and ((mag == 0) | ((mag >= 2.0 ** -14) & (mag < 65504.0))).all()
        t = torch.from_numpy(t32).to(_tdtype(torch, dtype))
        _LUT[consts, dtype] = t.view(torch.int32 if dtype == "float32" else torch.int16).numpy().copy()
    return _LUT[consts, dtype]


def bits_of(torch, t):
    """A float tensor's elements as integers, on the CPU."""
    t = t.contiguous().cpu()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


def expect_bits(table, px, flip=False):
    """[3, rh, rw] integer bits for the uint8 window px [rh, rw, >= 3]."""
    want = np.stack([table[px[:, :, c], c] for c in range(3)])
    return want[:, :, ::-1] if flip else want


# ---- 1..4. the kernel alone ------------------------------------------------------
def _merge_tensor(nice, ctx, imgs, tw, th, windows, dt, layout, leads, flips, consts, failed=(), stray=False,
                  raw_lead=None):
    """Every (window, tile) slot of `windows` in a shuffled order through
    nice_set_merge_tensor_dev into one poisoned buffer per window, with a guard
    row above and below, guard elements left and right and, planar, guard rows
    between the planes; the window's first element is `leads[j]` elements past
    a 16-byte boundary.  raw_lead: the slots are 3 bytes per pixel at byte
    offsets (d_src_off) that many bytes past a multiple of 16.  Returns each
    window's bits [3, rh, rw] and asserts the poison everywhere else."""
    import torch
    c = imgs[0].shape[2]
    es = 4 if dt == F32 else 2
    idt = torch.int32 if es == 4 else torch.int16
    poison = POISON_BITS[es]
    tiles = [np_tiles(im, tw, th) for im in imgs]
    slots = [(j, ti) for j, (i, x0, y0, rw, rh) in enumerate(windows)
             for ti in _touched(imgs[i].shape[1], imgs[i].shape[0], tw, th, x0, y0, rw, rh)]
    order = np.random.default_rng(len(slots)).permutation(len(slots))
    slots = [slots[k] for k in order]
    data = [tiles[windows[j][0]][ti] for j, ti in slots]
    status = [-5 if s in failed else 0 for s in slots]
    if stray:
        j = len(windows) - 1
        slots.append((j, tiles[windows[j][0]].shape[0] + 3))
        data.append(np.full((th, tw, c), 0x11, np.uint8))
        status.append(0)
    ns = len(slots)
    if raw_lead is None:
        tc = c
        stride = (tw * th * c + 15) // 16 * 16
        buf = torch.full((ns, stride), 0xA5, dtype=torch.uint8, device="cuda")
        buf[:, :tw * th * c] = torch.from_numpy(np.stack([d.reshape(-1) for d in data])).cuda()
        d_off = None
    else:
        tc = 3
        stride = (tw * th * 3 + 15) // 16 * 16 + 16
        host = np.full(ns * stride + 16, 0xA5, np.uint8)
        offs = [k * stride + raw_lead for k in range(ns)]
        for o, d in zip(offs, data):
            host[o:o + tw * th * 3] = d[:, :, :3].reshape(-1)
        buf = torch.from_numpy(host).cuda()
        d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    d_win = torch.tensor([j for j, _ in slots], dtype=torch.int32, device="cuda")
    d_tile = torch.tensor([ti for _, ti in slots], dtype=torch.int32, device="cuda")
    d_st = torch.tensor(status, dtype=torch.int32, device="cuda")
    bigs, ptrs, rps, pps, where = [], [], [], [], []
    for (i, x0, y0, rw, rh), lead in zip(windows, leads):
        n_el = rw if layout == PLANAR else 3 * rw
        row = (n_el + 7) // 8 * 8 + 24
        rows = rh + 3                                        # a guard row above, two below (between planes)
        big = torch.full((3 if layout == PLANAR else 1, rows, row), poison, dtype=idt, device="cuda")
        assert big.data_ptr() % 16 == 0
        bigs.append(big)
        ptrs.append(big.data_ptr() + (row + 8 + lead) * es)
        rps.append(row)
        pps.append(rows * row)
        where.append((slice(1, 1 + rh), slice(8 + lead, 8 + lead + n_el)))
    scale, bias = const_sets(nice)[consts]
    rc = nice.lib().nice_set_merge_tensor_dev(
        ctx.ptr, None, ctypes.c_void_p(buf.data_ptr()), 0 if d_off is not None else stride,
        ctypes.c_void_p(d_off.data_ptr()) if d_off is not None else None, ctypes.c_void_p(d_win.data_ptr()),
        ctypes.c_void_p(d_tile.data_ptr()), ctypes.c_void_p(d_st.data_ptr()) if failed else None, ns, tc,
        (ctypes.c_uint32 * len(imgs))(*[im.shape[1] for im in imgs]),
        (ctypes.c_uint32 * len(imgs))(*[im.shape[0] for im in imgs]), len(imgs), tw, th,
        (ctypes.c_uint32 * (5 * len(windows)))(*[v for wdw in windows for v in wdw]),
        (ctypes.c_uint8 * len(windows))(*[1 if f else 0 for f in flips]), (ctypes.c_void_p * len(windows))(*ptrs),
        (ctypes.c_uint64 * len(windows))(*rps), (ctypes.c_uint64 * len(windows))(*pps) if layout == PLANAR else None,
        len(windows), dt, layout, (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias))
    assert rc == 0
    torch.cuda.synchronize()
    outs = []
    for (i, x0, y0, rw, rh), big, (ys, xs) in zip(windows, bigs, where):
        got = big.cpu().numpy()
        win = got[:, ys, xs].copy()
        outs.append(win if layout == PLANAR else win.reshape(rh, rw, 3).transpose(2, 0, 1))
        got[:, ys, xs] = poison
        assert (got == poison).all(), (i, x0, y0, rw, rh)
    return outs, poison


def _expect_window(table, img, wdw, flip, tw, th, poison, failed_tiles=()):
    _, x0, y0, rw, rh = wdw
    want = expect_bits(table, img[y0:y0 + rh, x0:x0 + rw]).copy()          # unflipped, image order
    nx = -(-img.shape[1] // tw)
    for ti in failed_tiles:
        ty, tx = divmod(ti, nx)
        ya, yb = max(ty * th, y0) - y0, min((ty + 1) * th, y0 + rh) - y0
        xa, xb = max(tx * tw, x0) - x0, min((tx + 1) * tw, x0 + rw) - x0
        want[:, ya:yb, xa:xb] = poison
    return want[:, :, ::-1] if flip else want


# first element past a 16-byte boundary, in elements: 0 (the widest store that x0, or x0 + rw of a mirrored
# window, allows), 1 (element by element), 2 (stores of two elements at the most)
TENSOR_LEADS = [0, 1, 2, 0, 0, 2, 0, 1, 0]
TENSOR_FLIPS = [j % 2 for j in range(len(MERGE_WINDOWS))]


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("dt", [F32, F16, BF16])
@pytest.mark.parametrize("c", [4, 3])
@pytest.mark.parametrize("tw,th", [(64, 64), (66, 70)])
def test_merge_tensor_matches_table(nice, ctx, tw, th, c, dt, layout):
    imgs = [_random_image(w, h, c, i) for i, (w, h) in enumerate(MERGE_SHAPES)]
    table = lut_bits(nice, "odd", DTYPES[dt])
    outs, poison = _merge_tensor(nice, ctx, imgs, tw, th, MERGE_WINDOWS, dt, layout, TENSOR_LEADS, TENSOR_FLIPS, "odd")
    for wdw, flip, got in zip(MERGE_WINDOWS, TENSOR_FLIPS, outs):
        assert np.array_equal(got, _expect_window(table, imgs[wdw[0]], wdw, flip, tw, th, poison)), wdw


def plant_halfway(img, x0, y0, rw, rh):
    """The 14 (byte, channel) pairs of HALFWAY into the first pixels of the
    window, row by row: seven pixels hold them all, a smaller window what fits."""
    for i in range(min(7, rw * rh)):
        y, x = divmod(i, rw)
        img[y0 + y, x0 + x, :3] = [HALFWAY[c][i % len(HALFWAY[c])] for c in range(3)]


def holds_halfway(px):
    """Whether the pixels [rh, rw, >= 3] hold one of the (byte, channel) pairs of HALFWAY."""
    return any(np.isin(px[:, :, c], HALFWAY[c]).any() for c in range(3))


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("raw_lead", [None, 1])
def test_merge_tensor_float16_rounds_twice(nice, ctx, raw_lead, layout):
    """float16 on the constants whose elements differ between one rounding and
    two (tests/test_sets_tensor_cpu.py): the element is the float32 fmaf rounded
    again, in every store width (the leads give 1, 2 and 8 pixels per lane), for
    dense 4-byte slots and raw ones.  Every window holds such an element: the
    large ones among their random bytes, the small ones planted."""
    c = 4 if raw_lead is None else 3
    imgs = [_random_image(w, h, c, i) for i, (w, h) in enumerate(MERGE_SHAPES)]
    for i, x0, y0, rw, rh in MERGE_WINDOWS:
        if rw * rh < 100:                                  # 9 x 11, 3 x 7, 1 x 1
            plant_halfway(imgs[i], x0, y0, rw, rh)
    for i, x0, y0, rw, rh in MERGE_WINDOWS:
        assert rw * rh < 64 or holds_halfway(imgs[i][y0:y0 + rh, x0:x0 + rw]), (i, x0, y0)
    assert sum(rw * rh < 100 for _, _, _, rw, rh in MERGE_WINDOWS) == 3
    table = lut_bits(nice, "halfway", "float16")
    outs, poison = _merge_tensor(nice, ctx, imgs, 64, 64, MERGE_WINDOWS, F16, layout, TENSOR_LEADS, TENSOR_FLIPS, "halfway",
                                 raw_lead=raw_lead)
    for wdw, flip, got in zip(MERGE_WINDOWS, TENSOR_FLIPS, outs):
        assert np.array_equal(got, _expect_window(table, imgs[wdw[0]], wdw, flip, 64, 64, poison)), wdw


@pytest.mark.parametrize("flip", [0, 1])
def test_merge_tensor_long_row(nice, ctx, flip):
    imgs = [_random_image(700, 40, 4), _random_image(9, 20, 4, 1)]
    windows = [(0, 0, 0, 700, 40), (1, 0, 0, 9, 20), (0, 3, 17, 690, 20), (0, 8, 2, 688, 9)]
    table = lut_bits(nice, "imagenet", "float16")
    outs, poison = _merge_tensor(nice, ctx, imgs, 1024, 16, windows, F16, PLANAR, [0, 0, 0, 0], [flip] * 4, "imagenet")
    for wdw, got in zip(windows, outs):
        assert np.array_equal(got, _expect_window(table, imgs[wdw[0]], wdw, flip, 1024, 16, poison)), wdw


@pytest.mark.parametrize("dt,layout", [(F16, PLANAR), (F32, INTERLEAVED)])
def test_merge_tensor_skips_failed_and_stray_slots(nice, ctx, dt, layout):
    """A slot with a nonzero status and a tile index outside its image write nothing."""
    imgs = [_random_image(w, h, 4, i) for i, (w, h) in enumerate(MERGE_SHAPES)]
    windows = [(0, 0, 0, 200, 136), (1, 60, 4, 70, 66), (0, 50, 50, 100, 80)]
    failed = {(0, 6), (1, 1), (2, 5)}
    flips = [0, 1, 1]
    table = lut_bits(nice, "unit", DTYPES[dt])
    outs, poison = _merge_tensor(nice, ctx, imgs, 64, 64, windows, dt, layout, [0, 0, 2], flips, "unit", failed=failed,
                                 stray=True)
    for j, (wdw, got) in enumerate(zip(windows, outs)):
        lost = [ti for jj, ti in failed if jj == j]
        assert np.array_equal(got, _expect_window(table, imgs[wdw[0]], wdw, flips[j], 64, 64, poison, lost)), wdw


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
@pytest.mark.parametrize("raw_lead", [0, 4, 1])
def test_merge_tensor_raw_slots(nice, ctx, raw_lead, layout):
    """Raw slots through d_src_off, 3 bytes per pixel, rows 16- and 4-byte
    aligned and at an odd address: the values of coded slots of the same pixels."""
    imgs = [_random_image(w, h, 3, i) for i, (w, h) in enumerate(MERGE_SHAPES)]
    rgba = [np.concatenate([im, np.full(im.shape[:2] + (1,), 0x5A, np.uint8)], axis=2) for im in imgs]
    table = lut_bits(nice, "imagenet", "bfloat16")
    raw, poison = _merge_tensor(nice, ctx, imgs, 64, 64, MERGE_WINDOWS, BF16, layout, TENSOR_LEADS, TENSOR_FLIPS,
                                "imagenet", raw_lead=raw_lead)
    coded, _ = _merge_tensor(nice, ctx, rgba, 64, 64, MERGE_WINDOWS, BF16, layout, TENSOR_LEADS, TENSOR_FLIPS, "imagenet")
    for wdw, flip, a, b in zip(MERGE_WINDOWS, TENSOR_FLIPS, raw, coded):
        assert np.array_equal(a, b), wdw
        assert np.array_equal(a, _expect_window(table, imgs[wdw[0]], wdw, flip, 64, 64, poison)), wdw


# ---- 5. end to end on the reference set ---------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [3, 4])
def test_decode_all_images(nice, O, ctx, c, dtype):
    import torch
    r = ref(O, c)
    assert r.kind == [1 if t == 5 else 0 for t in range(46)]               # (test_sets.py: test_reference_set_counts)
    table = lut_bits(nice, "imagenet", dtype)
    scale, bias = const_sets(nice)["imagenet"]
    outs = nice.decode_set_tensor(encoded(nice, O, ctx, c), dtype=_tdtype(torch, dtype), scale=scale, bias=bias, ctx=ctx)
    assert last_set(nice, ctx) == (45, 1)
    assert len(outs) == K
    for im, out in zip(r.imgs, outs):
        assert tuple(out.shape) == (3,) + im.shape[:2] and out.dtype == _tdtype(torch, dtype) and out.is_contiguous()
        assert np.array_equal(bits_of(torch, out), expect_bits(table, im))
    # the default: float16, x / 255, and the allocated memory format
    outs = nice.decode_set_tensor(encoded(nice, O, ctx, c), images=[5, 3], channels_last=True, ctx=ctx)
    unit = lut_bits(nice, "unit", "float16")
    for i, out in zip([5, 3], outs):
        assert out.dtype == torch.float16 and out.stride(0) == 1 and (out.shape[2] == 1 or out.stride(2) == 3)
        assert np.array_equal(bits_of(torch, out), expect_bits(unit, r.imgs[i]))


def _crop_expect(nice, O, ctx, c, table):
    """The table lookup of decode_set's own uint8 crop batch, flipped as CROP_FLIPS; and its slot counts."""
    import torch
    u8 = torch.zeros((len(CROPS), 40, 48, 3), dtype=torch.uint8, device="cuda")
    nice.decode_set(encoded(nice, O, ctx, c), windows=CROPS, out=u8, ctx=ctx)
    counts = last_set(nice, ctx)
    px = u8.cpu().numpy()
    return np.stack([expect_bits(table, px[j], CROP_FLIPS[j]) for j in range(len(CROPS))]), counts


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("c", [3, 4])
def test_crop_batch(nice, O, ctx, c, channels_last):
    import torch
    r = ref(O, c)
    iset = encoded(nice, O, ctx, c)
    scale, bias = nice.normalize_affine((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    want, counts = _crop_expect(nice, O, ctx, c, lut_bits(nice, "imagenet", "float16"))
    out = torch.full((len(CROPS), 3, 40, 48), POISON, dtype=torch.float16, device="cuda")
    if channels_last:
        out = out.contiguous(memory_format=torch.channels_last)
        assert out.stride(1) == 1 and out.stride(3) == 3
    assert nice.decode_set_tensor(iset, windows=CROPS, out=out, scale=scale, bias=bias, flip=CROP_FLIPS, ctx=ctx) is out
    assert last_set(nice, ctx) == counts == _slot_counts(r, CROPS) and counts[1] == 2
    assert np.array_equal(bits_of(torch, out), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_crop_batch_into_strided_views(nice, O, ctx, dtype):
    """Views of poisoned larger tensors, planar and channels_last: nothing outside the views changes."""
    import torch
    iset = encoded(nice, O, ctx, 4)
    scale, bias = const_sets(nice)["imagenet"]
    want, _ = _crop_expect(nice, O, ctx, 4, lut_bits(nice, "imagenet", dtype))
    td = _tdtype(torch, dtype)
    m = len(CROPS)
    planar = torch.full((m, 4, 43, 53), POISON, dtype=td, device="cuda")
    nhwc = torch.full((m, 43, 53, 3), POISON, dtype=td, device="cuda")
    for big, view in ((planar, planar[:, 1:, 2:-1, 3:-2]), (nhwc, nhwc.permute(0, 3, 1, 2)[:, :, 2:-1, 3:-2])):
        assert tuple(view.shape) == (m, 3, 40, 48)
        assert nice.decode_set_tensor(iset, windows=CROPS, out=view, dtype=td, scale=scale, bias=bias, flip=CROP_FLIPS,
                                      ctx=ctx) is view
        assert np.array_equal(bits_of(torch, view), want)
        view.fill_(POISON)
        assert bool((big == POISON).all())
    # a list of views of different sizes, each in a buffer of its own
    small = [(3, 1, 2, 3, 4), (2, 60, 0, 5, 1), (0, 61, 59, 9, 11)]
    r = ref(O, 4)
    bigs = [torch.full((3, rh + 2, rw + 5), POISON, dtype=td, device="cuda") for _, _, _, rw, rh in small]
    views = [b[:, 1:-1, 3:-2] for b in bigs]
    back = nice.decode_set_tensor(iset, windows=small, out=views, dtype=td, scale=scale, bias=bias, flip=[0, 1, 1], ctx=ctx)
    assert all(a is b for a, b in zip(back, views))
    table = lut_bits(nice, "imagenet", dtype)
    for (i, x0, y0, rw, rh), f, big, view in zip(small, [0, 1, 1], bigs, views):
        assert np.array_equal(bits_of(torch, view), expect_bits(table, r.imgs[i][y0:y0 + rh, x0:x0 + rw], f)), (i, x0, y0)
        view.fill_(POISON)
        assert bool((big == POISON).all())


# ---- 6. a damaged tile ------------------------------------------------------------------
def test_damaged_tile_fails_alone(nice, O, ctx):
    """Bytes flipped in one coded tile of image 1: its slots fail, in every
    window that touches it, and keep the poison; everything else is written."""
    import torch
    r = ref(O, 4)
    iset = encoded(nice, O, ctx, 4)
    bad_ti = 7                                             # tile (1, 1) of image 1's 6 x 4 grid
    bad_t = r.first[1] + bad_ti
    assert r.kind[bad_t] == 0
    packed = iset.packed.clone()
    packed[int(iset.off[bad_t]) + 13 + 3] ^= 0xFF          # inside the table header, which follows the 13-byte file header
    hurt = dataclasses.replace(iset, packed=packed)
    table = lut_bits(nice, "unit", "float16")
    poison = int(bits_of(torch, torch.tensor([POISON], dtype=torch.float16))[0])
    outs = [torch.full((3,) + im.shape[:2], POISON, dtype=torch.float16, device="cuda") for im in r.imgs]
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set_tensor(hurt, out=outs, ctx=ctx)
    st = e.value.statuses
    assert len(st) == 46 and st[bad_t] < 0 and [s for t, s in enumerate(st) if t != bad_t] == [0] * 45
    assert all(a is b for a, b in zip(e.value.out, outs))
    for i, (im, out) in enumerate(zip(r.imgs, outs)):
        want = expect_bits(table, im).copy()
        if i == 1:
            want[:, 64:128, 64:128] = poison               # the damaged tile's elements keep the poison
        assert np.array_equal(bits_of(torch, out), want), i
    # two windows on that tile and one beside it: the tile fails once per window
    windows = [(1, 60, 60, 10, 10), (1, 70, 70, 20, 20), (1, 130, 70, 20, 20)]
    with pytest.raises(nice.NiceError) as e:
        nice.decode_set_tensor(hurt, windows=windows, flip=[1, 0, 1], ctx=ctx)
    st = e.value.statuses
    assert len(st) == 6 and [s < 0 for s in st] == [False, False, False, True, True, False]
    assert np.array_equal(bits_of(torch, e.value.out[2]), expect_bits(table, r.imgs[1][70:90, 130:150], True))
    # window 0, mirrored: its rows 0..3 hold columns 60..63 (the sound tile to the left) in output columns 9..6
    assert np.array_equal(bits_of(torch, e.value.out[0])[:, :4, 6:], expect_bits(table, r.imgs[1][60:64, 60:64], True))


# ---- 7. launch counts ----------------------------------------------------------------------
def test_launch_counts_do_not_depend_on_images_or_windows(nice, O):
    import torch
    ctx = nice.Context(0)
    imgs = _cuda(torch, ref(O, 4).imgs)
    one = nice.encode_set(imgs[:1], tile=(64, 64), ctx=ctx)
    six = nice.encode_set(imgs, tile=(64, 64), ctx=ctx)
    small = [(i, 0, 0, 5, 1) for i in range(K)] * 3
    L = nice.lib()
    L.nice_ctx_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.nice_ctx_set_timing(ctx.ptr, 1) == 0
    try:
        _timing(nice, ctx)
        counts = {}
        for name, fn in (("tensor", nice.decode_set_tensor), ("uint8", nice.decode_set)):
            fn(one, ctx=ctx)
            counts[name, "one"] = _timing(nice, ctx)
            fn(six, ctx=ctx)
            counts[name, "six"] = _timing(nice, ctx)
            fn(six, windows=small, ctx=ctx)
            counts[name, "windows"] = _timing(nice, ctx)
        t = counts["tensor", "one"]
        assert t[PH_DEC_TABLES] > 0 and t[PH_ENC_CLASSIFY] == 0
        for what in ("one", "six", "windows"):
            assert counts["tensor", what][PH_DEC_TABLES] == t[PH_DEC_TABLES], what
            assert counts["tensor", what][PH_DEC_TABLES] == counts["uint8", what][PH_DEC_TABLES], what
    finally:
        L.nice_ctx_set_timing(ctx.ptr, 0)


# ---- 8. rejections ---------------------------------------------------------------------------
def test_rejects(nice, O, ctx):
    import torch
    iset = encoded(nice, O, ctx, 3)
    two = [(0, 0, 0, 48, 40), (1, 0, 0, 48, 40)]

    def bad(**kw):
        with pytest.raises(nice.NiceError) as e:
            nice.decode_set_tensor(iset, ctx=ctx, **kw)
        assert e.value.code == E_ARG, kw

    def empty(*shape, dtype=torch.float16, device="cuda"):
        return torch.empty(shape, dtype=dtype, device=device)

    bad(dtype=torch.float64)
    bad(dtype=torch.uint8)
    for shape in ((2, 3, 48, 40), (3, 3, 40, 48), (2, 40, 48, 3), (2, 4, 40, 48), (2, 3, 40)):
        bad(windows=two, out=empty(*shape))
    bad(windows=two, out=[empty(3, 40, 48)])
    bad(windows=two, out=empty(2, 3, 40, 48, device="cpu"))
    bad(windows=two, out=empty(2, 3, 40, 48, dtype=torch.float32))                  # not the dtype asked for
    bad(windows=two, out=empty(2, 3, 40, 96)[:, :, :, ::2])                         # innermost stride 2: neither layout
    bad(windows=two, out=empty(2 * 4 * 40 * 48).as_strided((2, 3, 40, 48), (7680, 1, 192, 4)))     # channel stride 1, innermost 4
    bad(windows=two, out=[empty(3, 40, 48), empty(40, 48, 3).permute(2, 0, 1)])     # two layouts in one call
    bad(windows=two, out=empty(2 * 3 * 40 * 48).as_strided((2, 3, 40, 48), (5760, 1920, 47, 1)))   # row pitch < rw
    bad(windows=two, out=empty(2 * 3 * 40 * 48).as_strided((2, 3, 40, 48), (5760, 1, 143, 3)))     # row pitch < 3 rw
    bad(windows=two, flip=[1])
    bad(windows=two, flip=[1, 0, 1])
    bad(scale=(float("inf"), 1, 1))
    bad(bias=(0, float("nan"), 0))
    bad(scale=(1e39, 1, 1))                                                         # infinite once rounded to float32
    bad(scale=(1, 1))
    bad(images=[0], windows=two)
    bad(images=[K])
    bad(windows=[(0, 150, 100, 51, 1)])
    bad(flags=nice.DEC_STRICT_REFERENCE)
    # the C entry points: an unknown dtype or layout, null or non-finite constants, a misaligned base
    L = nice.lib()
    out = empty(2, 3, 40, 48)
    st = torch.zeros(64, dtype=torch.int32, device="cuda")
    off, lens, kind = iset.off.contiguous(), iset.stream_len.contiguous(), iset.kind.contiguous()
    n = iset.first[-1]
    one = (ctypes.c_float * 3)(1, 1, 1)
    inf = (ctypes.c_float * 3)(1, float("inf"), 1)

    def call(dt=F16, layout=PLANAR, scale=one, bias=one, base=0, flags=0):
        return L.nice_decode_set_tensor_dev(
            ctx.ptr, None, ctypes.c_void_p(iset.packed.data_ptr()), int(off[n]), ctypes.c_void_p(off.data_ptr()),
            ctypes.c_void_p(lens.data_ptr()), ctypes.c_void_p(kind.data_ptr()),
            (ctypes.c_uint32 * K)(*iset.widths), (ctypes.c_uint32 * K)(*iset.heights), K, 64, 64,
            (ctypes.c_uint32 * 10)(*[v for w in two for v in w]), None,
            (ctypes.c_void_p * 2)(out[0].data_ptr() + base, out[1].data_ptr() + base),
            (ctypes.c_uint64 * 2)(48, 48), (ctypes.c_uint64 * 2)(1920, 1920), 2, dt, layout, scale, bias, flags,
            ctypes.c_void_p(st.data_ptr()))

    assert call(dt=3) == E_ARG and call(layout=2) == E_ARG
    assert call(scale=None) == E_ARG and call(bias=None) == E_ARG and call(scale=inf) == E_ARG and call(bias=inf) == E_ARG
    assert call(base=1) == E_ARG and call(dt=F32, base=2) == E_ARG
    assert call(flags=nice.DEC_STRICT_REFERENCE) == E_ARG
    assert call(layout=INTERLEAVED) == E_ARG                                        # row pitch 48 < 3 * 48
    assert call() == 0
    torch.cuda.synchronize()


# ---- 9. decode_set is untouched ------------------------------------------------------------------
def test_decode_set_is_untouched(nice, O, ctx):
    import torch
    iset = encoded(nice, O, ctx, 4)
    before = nice.decode_set(iset, windows=CROPS, ctx=ctx)
    counts = last_set(nice, ctx)
    nice.decode_set_tensor(iset, windows=CROPS, flip=CROP_FLIPS, dtype=torch.bfloat16, channels_last=True, ctx=ctx)
    after = nice.decode_set(iset, windows=CROPS, ctx=ctx)
    assert last_set(nice, ctx) == counts
    for a, b, (i, x0, y0, rw, rh) in zip(before, after, CROPS):
        assert torch.equal(a, b) and tuple(b.shape) == (rh, rw, 4)
        assert np.array_equal(b.cpu().numpy()[:, :, :3], ref(O, 4).imgs[i][y0:y0 + rh, x0:x0 + rw, :3])
        assert bool((b[:, :, 3] == 255).all())
