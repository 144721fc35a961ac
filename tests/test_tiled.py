"""Tiled images on the GPU (include/nice.h, "tiled images"): the split and merge
kernels against numpy on random bytes, the tiled encode against the oracle tile
by tile (streams byte for byte, raw tiles exactly where the oracle's tolerant
decode fails or differs), the decode of whole images and regions, a damaged
tile, the container and the command line.

Expected tiles are built in numpy with the clamp rule: a tile position outside
the image takes the pixel at (min(x, w - 1), min(y, h - 1))."""
import ctypes
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


def np_tiles(img, tw, th):
    """[h, w, c] -> [n, th, tw, c], tile t = ty * nx + tx, padded by the clamp rule."""
    h, w, c = img.shape
    nx, ny = -(-w // tw), -(-h // th)
    ys = np.minimum(np.arange(ny * th), h - 1)
    xs = np.minimum(np.arange(nx * tw), w - 1)
    big = img[ys][:, xs]
    return np.ascontiguousarray(big.reshape(ny, th, nx, tw, c).transpose(0, 2, 1, 3, 4).reshape(nx * ny, th, tw, c))


def crafted_image(O, c):
    """200 x 136 SYN-v1 seed 5 whose pixels [64:128, 64:128] (tile 5 of the
    64 x 64 grid) are a gradient with 16 small-difference pixels: that tile's
    small-difference table gets a 131-bit longest code, which no decoder can
    read back from the table header."""
    img = O.gen_syn_v1(200, 136, c, 5).reshape(136, 200, c).copy()
    px = O.gen_gradient(64, 64, c).reshape(64, 64, c).copy()
    rng = np.random.default_rng(16)
    for i in range(16):
        y = rng.integers(4, 63)
        x = rng.integers(4, 60)
        px[y, x, :3] = px[y, x - 1, :3] + np.array([1 + i % 3, (i // 3) % 3, 2], np.uint8)
    img[64:128, 64:128] = px
    return img


# name: (w, h, c, tile_w, tile_h, image source)
CASES = {
    "crafted3": (200, 136, 3, 64, 64, "crafted"),     # right and bottom edges of 8 pixels, one raw tile
    "crafted4": (200, 136, 4, 64, 64, "crafted"),
    "odd": (333, 211, 3, 66, 70, 3),                  # nothing aligned
    "row": (65, 1, 3, 64, 64, 4),
    "tiny": (5, 7, 4, 64, 64, 6),                     # smaller than one tile
    "exact": (64, 64, 4, 64, 64, 7),                  # one tile, no padding
}


class Ref:
    """One case's image, padded tiles and the oracle's stream and verdict per
    tile; built once and left unchanged."""

    def __init__(self, O, name):
        self.w, self.h, self.c, self.tw, self.th, src = CASES[name]
        w, h, c = self.w, self.h, self.c
        self.img = crafted_image(O, c) if src == "crafted" else O.gen_syn_v1(w, h, c, src).reshape(h, w, c)
        self.tiles = np_tiles(self.img, self.tw, self.th)
        self.nx, self.ny = -(-w // self.tw), -(-h // self.th)
        self.streams, self.kind = [], []
        for t in self.tiles:
            s, k = oracle_verdict(O, t)
            self.streams.append(s)
            self.kind.append(k)


def oracle_verdict(O, tile):
    """(oracle stream, 0 if the oracle's tolerant decode returns the tile's RGB, else 1)."""
    th, tw, c = tile.shape
    s = O.encode(tile, tw, th, c)
    try:
        px, _ = O.decode(s, O.DEC_TOLERANT)
        ok = np.array_equal(px.reshape(-1, c)[:, :3], tile.reshape(-1, c)[:, :3])
    except O.OracleDecodeError:
        ok = False
    return s, 0 if ok else 1


_REFS = {}


def ref(O, name):
    if name not in _REFS:
        _REFS[name] = Ref(O, name)
    return _REFS[name]


@pytest.fixture(scope="module")
def ctx(nice):
    return nice.Context(0)


def last_tiled(nice, ctx):
    L = nice.lib()
    L.nice_test_last_tiled.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.nice_test_last_tiled(ctx.ptr, ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value, b.value


def device_image(torch, img, pitch_extra=0, base_off=0):
    """`img` on the GPU as a row-strided view: rows of w*c + pitch_extra bytes,
    the first pixel base_off bytes past a 256-byte boundary.  Poison around it."""
    h, w, c = img.shape
    pitch = w * c + pitch_extra
    raw = torch.full((h * pitch + base_off + 64,), POISON, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 256 == 0
    view = raw[base_off:base_off + h * pitch].view(h, pitch)[:, :w * c].view(h, w, c)
    view.copy_(torch.from_numpy(np.ascontiguousarray(img)).cuda())
    assert view.data_ptr() % 256 == base_off and (h == 1 or view.stride(0) == pitch)
    return raw, view


# ---- 1. split and merge alone, on random bytes -------------------------------
# (w, h, c, tile_w, tile_h, pitch_extra, base_off)
COPY_CASES = [
    (200, 136, 3, 64, 64, 0, 0), (200, 136, 4, 64, 64, 0, 0),      # RGBA: pitch 800, the 16-byte path
    (333, 211, 3, 66, 70, 0, 0), (65, 1, 3, 64, 64, 0, 0), (5, 7, 4, 64, 64, 0, 0),
    (200, 136, 3, 64, 64, 12, 0), (200, 136, 4, 64, 64, 12, 0),    # row_pitch = w*c + 12: dwords for RGBA
    (200, 136, 4, 64, 64, 32, 0),                                  # pitched and still 16-byte aligned
    (200, 136, 4, 64, 64, 0, 4),                                   # the same image 4 bytes on: dwords
    (200, 136, 4, 64, 64, 0, 1),                                   # any base: bytes
    (200, 136, 4, 66, 64, 0, 0),                                   # tile_w % 4 != 0: dwords
    (700, 40, 4, 1024, 16, 0, 0),                                  # a row longer than one unrolled step
]


def _random_image(w, h, c):
    return np.random.default_rng(w * 31 + h * 7 + c).integers(0, 256, (h, w, c), dtype=np.uint8)


@pytest.mark.parametrize("w,h,c,tw,th,pitch_extra,base_off", COPY_CASES)
def test_split_matches_numpy(nice, ctx, w, h, c, tw, th, pitch_extra, base_off):
    import torch
    img = _random_image(w, h, c)
    want = np_tiles(img, tw, th)
    n = want.shape[0]
    raw, view = device_image(torch, img, pitch_extra, base_off)
    pitch = w * c + pitch_extra
    for stride_extra in (0, 16) if base_off == 0 else (0,):
        stride = (tw * th * c + 15) // 16 * 16 + stride_extra
        tiles = torch.full((n * stride + 64,), POISON, dtype=torch.uint8, device="cuda")
        rc = nice.lib().nice_tiles_split_dev(ctx.ptr, None, ctypes.c_void_p(view.data_ptr()), pitch, w, h, c, tw, th,
                                             ctypes.c_void_p(tiles.data_ptr()), stride)
        assert rc == 0
        torch.cuda.synchronize()
        got = tiles.cpu().numpy()
        slots = got[:n * stride].reshape(n, stride)
        assert np.array_equal(slots[:, :tw * th * c].reshape(want.shape), want)
        assert (slots[:, tw * th * c:] == POISON).all() and (got[n * stride:] == POISON).all()


def _rois(w, h, tw, th):
    rois = [(0, 0, w, h), (w - 1, h - 1, 1, 1)]
    if w > tw + 9 and h > th + 9:
        rois += [(tw - 3, th - 5, 9, 11), (4, 3, w - 7, h - 5), (tw, th, min(tw, w - tw), min(th, h - th)),
                 (8, 0, w - 8, h)]
    return rois


@pytest.mark.parametrize("w,h,c,tw,th,pitch_extra,base_off", COPY_CASES)
def test_merge_matches_numpy(nice, ctx, w, h, c, tw, th, pitch_extra, base_off):
    """Slots in a shuffled order, merged into a window inside a poisoned larger
    tensor: the window is the image's rectangle, not a byte around it changes."""
    import torch
    img = _random_image(w, h, c)
    tiles_np = np_tiles(img, tw, th)
    n = tiles_np.shape[0]
    order = np.random.default_rng(n).permutation(n)
    stride = (tw * th * c + 15) // 16 * 16
    slots = torch.full((n, stride), POISON, dtype=torch.uint8, device="cuda")
    slots[:, :tw * th * c] = torch.from_numpy(tiles_np[order].reshape(n, -1)).cuda()
    idx = torch.from_numpy(order.astype(np.int32)).cuda()
    for x0, y0, rw, rh in _rois(w, h, tw, th):
        for oc in (3, 4):
            opitch = rw * oc + pitch_extra + (0 if oc == 3 else (-rw * oc) % 16)
            big = torch.full((rh + 2, opitch + 48), POISON, dtype=torch.uint8, device="cuda")
            lead = 16 + base_off
            win = big[1:1 + rh, lead:lead + rw * oc]
            rc = nice.lib().nice_tiles_merge_dev(ctx.ptr, None, ctypes.c_void_p(slots.data_ptr()), stride,
                                                 ctypes.c_void_p(idx.data_ptr()), n, c, w, h, tw, th, x0, y0, rw, rh,
                                                 oc, 0x7E, ctypes.c_void_p(win.data_ptr()), big.stride(0))
            assert rc == 0
            torch.cuda.synchronize()
            got = big.cpu().numpy()
            g = got[1:1 + rh, lead:lead + rw * oc].reshape(rh, rw, oc)
            want = img[y0:y0 + rh, x0:x0 + rw]
            assert np.array_equal(g[:, :, :3], want[:, :, :3]), (x0, y0, rw, rh, oc)
            if oc == 4:
                assert np.array_equal(g[:, :, 3], want[:, :, 3] if c == 4 else np.full((rh, rw), 0x7E)), (x0, y0, oc)
            got[1:1 + rh, lead:lead + rw * oc] = POISON
            assert (got == POISON).all(), (x0, y0, rw, rh, oc)


def test_merge_subset_and_bad_index(nice, ctx):
    """Only the listed slots are written; an index past the grid is skipped."""
    import torch
    w, h, c, tw, th = 200, 136, 4, 64, 64
    img = _random_image(w, h, c)
    tiles_np = np_tiles(img, tw, th)
    pick = np.array([6, 99, 1], np.int32)
    slots = torch.from_numpy(np.stack([tiles_np[6], tiles_np[0], tiles_np[1]]).reshape(3, -1)).cuda()
    out = torch.full((h, w, c), POISON, dtype=torch.uint8, device="cuda")
    rc = nice.lib().nice_tiles_merge_dev(ctx.ptr, None, ctypes.c_void_p(slots.data_ptr()), slots.stride(0),
                                         ctypes.c_void_p(torch.from_numpy(pick).cuda().data_ptr()), 3, c, w, h, tw, th,
                                         0, 0, w, h, c, 0, ctypes.c_void_p(out.data_ptr()), w * c)
    assert rc == 0
    torch.cuda.synchronize()
    want = np.full((h, w, c), POISON, np.uint8)
    want[64:128, 128:192] = img[64:128, 128:192]
    want[0:64, 64:128] = img[0:64, 64:128]
    assert np.array_equal(out.cpu().numpy(), want)


# ---- 2. encode ---------------------------------------------------------------
def test_crafted_tile_is_outside_the_format(O):
    """The precondition of the raw-tile cases: the oracle cannot decode tile 5
    of the crafted image and decodes the other 11 exactly."""
    for name in ("crafted3", "crafted4"):
        r = ref(O, name)
        _, st = O.encode(r.tiles[5], 64, 64, r.c, with_stats=True)
        assert st.max_aob[5] == 131
        with pytest.raises(O.OracleDecodeError):
            O.decode(r.streams[5], O.DEC_TOLERANT)
        assert r.kind == [1 if t == 5 else 0 for t in range(12)]


def _check_encoded(nice, r, timg):
    n = r.nx * r.ny
    assert (timg.nx, timg.ny, timg.width, timg.height, timg.channels) == (r.nx, r.ny, r.w, r.h, r.c)
    lens, off, kind = timg.stream_len.numpy(), timg.off.numpy(), timg.kind.numpy()
    assert off.shape == (n + 1,) and off[0] == 0 and np.array_equal(np.diff(off), (lens + 15) // 16 * 16)
    assert timg.packed.numel() == off[n] == timg.nbytes
    blob = timg.packed.cpu().numpy()
    assert kind.tolist() == r.kind        # 1 exactly where the oracle's tolerant decode raises or differs
    for t in range(n):
        s = blob[off[t]:off[t] + lens[t]].tobytes()
        if kind[t] == 0:
            assert s == r.streams[t], t
        else:
            assert s == r.tiles[t][:, :, :3].tobytes(), t
        assert not blob[off[t] + lens[t]:off[t + 1]].any(), t


_ENC = {}


def encoded(nice, O, ctx, name):
    """The case's TiledImage, encoded once."""
    import torch
    if name not in _ENC:
        r = ref(O, name)
        _ENC[name] = nice.encode_tiled(torch.from_numpy(r.img).cuda(), tile=(r.tw, r.th), ctx=ctx)
    return _ENC[name]


@pytest.mark.parametrize("name", list(CASES))
def test_encode_matches_oracle(nice, O, ctx, name):
    r = ref(O, name)
    timg = encoded(nice, O, ctx, name)
    _check_encoded(nice, r, timg)
    if name.startswith("crafted"):
        assert timg.kind.tolist() == [1 if t == 5 else 0 for t in range(12)]


@pytest.mark.parametrize("pitch_extra,base_off", [(12, 0), (32, 0), (0, 4)])
def test_encode_pitched_input(nice, O, ctx, pitch_extra, base_off):
    import torch
    r = ref(O, "crafted4")
    raw, view = device_image(torch, r.img, pitch_extra, base_off)
    _check_encoded(nice, r, nice.encode_tiled(view, tile=(r.tw, r.th), ctx=ctx))
    assert (raw.view(-1)[:base_off] == POISON).all()     # (the input is only read)


def test_encode_capacity(nice, O, ctx):
    import torch
    r = ref(O, "crafted3")
    need = encoded(nice, O, ctx, "crafted3").nbytes
    px = torch.from_numpy(r.img).cuda()
    buf = torch.full((need + 64,), POISON, dtype=torch.uint8, device="cuda")
    with pytest.raises(nice.NiceError) as e:
        nice.encode_tiled(px, tile=(64, 64), ctx=ctx, packed=buf[:need - 16])
    assert e.value.code == E_CAPACITY
    assert bool((buf[need - 16:] == POISON).all())
    _check_encoded(nice, r, nice.encode_tiled(px, tile=(64, 64), ctx=ctx, packed=buf[:need]))
    assert bool((buf[need:] == POISON).all())
    with pytest.raises(nice.NiceError) as e:
        nice.encode_tiled(px, tile=(1, 64), ctx=ctx)
    assert e.value.code == E_ARG


# ---- 3. decode, full image ---------------------------------------------------
@pytest.mark.parametrize("oc", [3, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_decode_full(nice, O, ctx, name, oc):
    r = ref(O, name)
    out = nice.decode_tiled(encoded(nice, O, ctx, name), out_channels=oc, ctx=ctx)
    assert tuple(out.shape) == (r.h, r.w, oc)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :, :3], r.img[:, :, :3])
    if oc == 4:
        assert (got[:, :, 3] == 255).all()
    assert sum(last_tiled(nice, ctx)) == r.nx * r.ny


def test_decode_alpha_without_fill(nice, O, ctx):
    out = nice.decode_tiled(encoded(nice, O, ctx, "crafted3"), out_channels=4, flags=0, ctx=ctx).cpu().numpy()
    assert np.array_equal(out[:, :, :3], ref(O, "crafted3").img) and (out[:, :, 3] == 0).all()


# ---- 4. decode, regions --------------------------------------------------------
# roi, (coded, raw) tiles it selects on the 4 x 3 grid whose tile 5 is raw
ROIS = [((10, 10, 30, 20), (1, 0)),         # inside one tile
        ((70, 70, 20, 30), (0, 1)),         # inside the raw tile
        ((61, 59, 9, 11), (3, 1)),          # across four tiles, odd corners
        ((50, 50, 100, 80), (8, 1)),        # the raw tile and its neighbours
        ((64, 64, 64, 64), (0, 1)),         # corners on tile edges
        ((199, 135, 1, 1), (1, 0)),
        ((0, 0, 200, 136), (11, 1))]


@pytest.mark.parametrize("name", ["crafted3", "crafted4"])
@pytest.mark.parametrize("roi,counts", ROIS)
def test_decode_region(nice, O, ctx, name, roi, counts):
    import torch
    r = ref(O, name)
    timg = encoded(nice, O, ctx, name)
    x0, y0, rw, rh = roi
    want = r.img[y0:y0 + rh, x0:x0 + rw, :3]
    for oc in (3, 4):
        out = nice.decode_tiled(timg, roi=roi, out_channels=oc, ctx=ctx)
        assert last_tiled(nice, ctx) == counts            # only the selected tiles were decoded
        assert tuple(out.shape) == (rh, rw, oc)
        assert np.array_equal(out.cpu().numpy()[:, :, :3], want), (roi, oc)
    # a row-strided out inside a poisoned larger tensor
    big = torch.full((rh + 2, rw + 5, r.c), POISON, dtype=torch.uint8, device="cuda")
    win = big[1:1 + rh, 3:3 + rw]
    assert nice.decode_tiled(timg, roi=roi, out=win, ctx=ctx) is win
    got = big.cpu().numpy()
    assert np.array_equal(got[1:1 + rh, 3:3 + rw, :3], want)
    got[1:1 + rh, 3:3 + rw] = POISON
    assert (got == POISON).all()


def test_decode_region_rejects(nice, O, ctx):
    timg = encoded(nice, O, ctx, "crafted3")
    for roi in ((200, 0, 1, 1), (0, 136, 1, 1), (0, 0, 0, 1), (0, 0, 1, 0), (150, 100, 51, 1), (150, 100, 1, 37)):
        with pytest.raises(nice.NiceError) as e:
            nice.decode_tiled(timg, roi=roi, ctx=ctx)
        assert e.value.code == E_ARG, roi
    with pytest.raises(nice.NiceError) as e:
        nice.decode_tiled(timg, flags=nice.DEC_STRICT_REFERENCE, ctx=ctx)
    assert e.value.code == E_ARG


# ---- 5. a damaged tile -------------------------------------------------------
def test_damaged_tile_fails_alone(nice, O, ctx):
    import dataclasses
    import torch
    r = ref(O, "crafted4")
    timg = encoded(nice, O, ctx, "crafted4")
    bad_t = 6
    packed = timg.packed.clone()
    packed[int(timg.off[bad_t]) + 13 + 3] ^= 0xFF          # inside the table header, which follows the 13-byte file header
    hurt = dataclasses.replace(timg, packed=packed)
    out = torch.full((r.h, r.w, 4), POISON, dtype=torch.uint8, device="cuda")
    with pytest.raises(nice.NiceError) as e:
        nice.decode_tiled(hurt, out=out, ctx=ctx)
    st = e.value.statuses
    assert len(st) == 12 and st[bad_t] < 0 and [s for t, s in enumerate(st) if t != bad_t] == [0] * 11
    got = out.cpu().numpy()
    assert (got[64:128, 128:192] == POISON).all()          # tile 6's pixels keep the poison
    want = np.concatenate([r.img[:, :, :3], np.full((r.h, r.w, 1), 255, np.uint8)], axis=2)
    want[64:128, 128:192] = POISON
    assert np.array_equal(got, want)
    # a raw tile of the wrong length, and a kind that is neither
    lens = timg.stream_len.clone()
    lens[5] -= 1
    kind = timg.kind.clone()
    kind[0] = 2
    with pytest.raises(nice.NiceError) as e:
        nice.decode_tiled(dataclasses.replace(timg, stream_len=lens, kind=kind), roi=(0, 0, 128, 128), ctx=ctx)
    assert e.value.statuses == [nice.E_FORMAT, 0, 0, nice.E_FORMAT]
    assert np.array_equal(e.value.out.cpu().numpy()[64:128, 0:64, :3], r.img[64:128, 0:64, :3])


# ---- 6. one real-size case ---------------------------------------------------
def test_real_size(nice, O, ctx):
    import torch
    w, h, c, tw, th = 1100, 700, 4, 512, 256
    img = O.gen_syn_v1(w, h, c, 2).reshape(h, w, c)
    tiles = np_tiles(img, tw, th)
    timg = nice.encode_tiled(torch.from_numpy(img).cuda(), tile=(tw, th), ctx=ctx)
    assert (timg.nx, timg.ny) == (3, 3)
    assert timg.kind.tolist() == [0] * 9
    blob, off, lens = timg.packed.cpu().numpy(), timg.off.numpy(), timg.stream_len.numpy()
    for t in (0, 5, 8):                                    # interior, right edge, the corner: both paddings
        s, k = oracle_verdict(O, tiles[t])
        assert k == 0 and blob[off[t]:off[t] + lens[t]].tobytes() == s, t
    out = nice.decode_tiled(timg, ctx=ctx).cpu().numpy()
    assert np.array_equal(out[:, :, :3], img[:, :, :3]) and (out[:, :, 3] == 255).all()
    roi = (500, 250, 30, 20)
    assert np.array_equal(nice.decode_tiled(timg, roi=roi, out_channels=3, ctx=ctx).cpu().numpy(),
                          img[250:270, 500:530, :3])
    assert last_tiled(nice, ctx) == (4, 0)


# ---- 7. container and CLI ----------------------------------------------------
def test_container_round_trip(nice, O, ctx, tmp_path):
    import torch
    r = ref(O, "crafted4")
    timg = encoded(nice, O, ctx, "crafted4")
    path = str(tmp_path / "img.nicet")
    nice.save_tiled(path, timg)
    back = nice.load_tiled(path, device="cuda")
    assert back.packed.is_cuda and torch.equal(back.packed, timg.packed)
    assert torch.equal(back.off, timg.off) and torch.equal(back.kind, timg.kind)
    out = nice.decode_tiled(back, out_channels=3, ctx=ctx).cpu().numpy()
    assert np.array_equal(out, r.img[:, :, :3])
    cpu = nice.load_tiled(path)
    assert not cpu.packed.is_cuda
    with pytest.raises(nice.NiceError) as e:
        nice.decode_tiled(cpu, ctx=ctx)
    assert e.value.code == E_ARG


def test_cli_png_nicet_png(nice, O, tmp_path, c=4):
    """(an RGBA PNG: one case, three processes)"""
    png = importlib.import_module(PKG_NAME + ".png")
    r = ref(O, f"crafted{c}")
    src = str(tmp_path / "in.png")
    png.write_png(src, r.img.reshape(-1), r.w, r.h, c)
    run = subprocess.run([sys.executable, CLI, src, str(tmp_path / "out"), "--tile", "64x64"], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stderr
    assert "tiles: 4x3 raw: 1" in run.stdout
    timg = nice.load_tiled(str(tmp_path / "out.nicet"))
    assert timg.kind.tolist() == r.kind and (timg.tile_w, timg.tile_h, timg.channels) == (64, 64, c)
    run = subprocess.run([sys.executable, CLI, str(tmp_path / "out.nicet"), str(tmp_path / "back")],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got, gw, gh, gc = png.read_png(str(tmp_path / "back.png"))
    assert (gw, gh, gc) == (r.w, r.h, 3) and np.array_equal(got.reshape(r.h, r.w, 3), r.img[:, :, :3])
    run = subprocess.run([sys.executable, CLI, str(tmp_path / "out.nicet"), str(tmp_path / "part.png"), "--roi",
                          "61,59,70,11"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got, gw, gh, gc = png.read_png(str(tmp_path / "part.png"))
    assert (gw, gh, gc) == (70, 11, 3) and np.array_equal(got.reshape(11, 70, 3), r.img[59:70, 61:131, :3])
