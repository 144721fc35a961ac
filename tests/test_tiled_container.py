"""Tiled images without a GPU: the grid and tile-selection arithmetic of the C
ABI (nice_tile_grid / nice_tile_select) against a brute-force numpy model, and
the NICETILE container (save_tiled / load_tiled) on CPU tensors."""
import struct

import numpy as np
import pytest

HEADER = "<8sIIIIIIIIIQ"   # magic, version, width, height, channels, tile_w, tile_h, nx, ny, reserved, packed size
HSZ = struct.calcsize(HEADER)
E_ARG, E_FORMAT = -1, -5


def _labels(w, h, tw, th):
    """Tile index of every image pixel, written out pixel by pixel."""
    xs, ys = np.arange(w) // tw, np.arange(h) // th
    nx = int(xs.max()) + 1
    return ys[:, None] * nx + xs[None, :], nx, int(ys.max()) + 1


# (w, h, tile_w, tile_h): w < tile_w, w % tile_w == 1, exact multiples, a 2 x 2 tile, a one-row image
GEOMS = [(5, 7, 64, 64), (65, 1, 64, 64), (200, 136, 64, 64), (129, 70, 64, 35), (128, 128, 64, 64), (333, 211, 66, 70),
         (9, 9, 2, 2), (64, 64, 64, 64)]


@pytest.mark.parametrize("w,h,tw,th", GEOMS)
def test_grid_and_select_match_brute_force(nice, w, h, tw, th):
    lab, nx, ny = _labels(w, h, tw, th)
    assert nice.tile_grid(w, h, tw, th) == (nx, ny)
    assert nice.tiled_bound(w, h, tw, th) == nice.packed_bound(nx * ny, tw, th)
    rng = np.random.default_rng(w * 1000 + h)
    rects = [(0, 0, w, h), (w - 1, h - 1, 1, 1), (0, 0, 1, 1)]
    # corners on and next to every tile edge
    ex = sorted({min(max(e + d, 0), w - 1) for e in range(0, w + tw, tw) for d in (-1, 0, 1)})
    ey = sorted({min(max(e + d, 0), h - 1) for e in range(0, h + th, th) for d in (-1, 0, 1)})
    for x0 in ex:
        for y0 in ey:
            x1 = int(rng.choice([x for x in ex if x >= x0])) + 1
            y1 = int(rng.choice([y for y in ey if y >= y0])) + 1
            rects.append((x0, y0, x1 - x0, y1 - y0))
    for x0, y0, rw, rh in rects:
        tx0, ty0, tx1, ty1 = nice.tile_select(w, h, tw, th, x0, y0, rw, rh)
        want = set(np.unique(lab[y0:y0 + rh, x0:x0 + rw]).tolist())
        got = {ty * nx + tx for ty in range(ty0, ty1) for tx in range(tx0, tx1)}
        assert got == want, (x0, y0, rw, rh)


def test_rejected_geometry_and_rectangles(nice):
    def refused(fn, *a):
        with pytest.raises(nice.NiceError) as e:
            fn(*a)
        assert e.value.code == E_ARG, a

    for tw, th in ((1, 64), (64, 1), (8193, 64), (64, 8193), (0, 0)):
        refused(nice.tile_grid, 200, 136, tw, th)
        assert nice.tiled_bound(200, 136, tw, th) == 0
    refused(nice.tile_grid, 0, 10, 64, 64)
    refused(nice.tile_grid, 10, 0, 64, 64)
    refused(nice.tile_grid, 32768, 32769, 64, 64)          # more than 2^30 pixels
    assert nice.tile_grid(32768, 32768, 8192, 8192) == (4, 4)
    assert nice.tile_grid(32768, 32768, 2, 2) == (16384, 16384)   # 2^28 tiles of one encoder tile each
    for rect in ((0, 0, 0, 5), (0, 0, 5, 0), (200, 0, 1, 1), (0, 136, 1, 1), (199, 135, 2, 1), (199, 135, 1, 2),
                 (0, 0, 201, 1), (0, 0, 1, 137), (2**32 - 1, 0, 2, 1), (2**31, 2**31, 2**31, 2**31)):
        refused(nice.tile_select, 200, 136, 64, 64, *rect)


def _fake(torch, nice, w=200, h=136, c=3, tw=64, th=64, raw=(5,)):
    """A TiledImage of fake streams in the packed layout, tile 5 raw."""
    rng = np.random.default_rng(3)
    nx, ny = -(-w // tw), -(-h // th)
    n = nx * ny
    lens = rng.integers(20, 900, n).astype(np.int64)
    kind = np.zeros(n, np.uint8)
    for t in raw:
        lens[t], kind[t] = tw * th * 3, 1
    off = np.zeros(n + 1, np.int64)
    np.cumsum((lens + 15) // 16 * 16, out=off[1:])
    blob = np.zeros(int(off[-1]), np.uint8)
    for t in range(n):
        blob[off[t]:off[t] + lens[t]] = rng.integers(1, 256, lens[t], dtype=np.uint8)
    return nice.TiledImage(w, h, c, tw, th, torch.from_numpy(blob), torch.from_numpy(off), torch.from_numpy(lens),
                           torch.from_numpy(kind))


def _write(path, t, **kw):
    """The container written out by hand, any field replaced through kw."""
    n = t.nx * t.ny
    f = dict(magic=b"NICETILE", version=1, width=t.width, height=t.height, channels=t.channels, tile_w=t.tile_w,
             tile_h=t.tile_h, nx=t.nx, ny=t.ny, reserved=0, size=int(t.off[n]), lens=t.stream_len.numpy(),
             offs=t.off.numpy(), kinds=t.kind.numpy(), blob=t.packed.numpy().tobytes())
    f.update(kw)
    with open(path, "wb") as fh:
        fh.write(struct.pack(HEADER, f["magic"], f["version"], f["width"], f["height"], f["channels"], f["tile_w"],
                             f["tile_h"], f["nx"], f["ny"], f["reserved"], f["size"]))
        fh.write(np.asarray(f["lens"], "<u8").tobytes())
        fh.write(np.asarray(f["offs"], "<u8").tobytes())
        k = np.asarray(f["kinds"], np.uint8).tobytes()
        fh.write(k + bytes(-len(k) % 8))
        fh.write(f["blob"])


def test_container_round_trip_and_rejects(nice, tmp_path):
    import torch
    t = _fake(torch, nice)
    assert (t.nx, t.ny) == (4, 3) and t.nbytes == int(t.off[12])
    path = str(tmp_path / "img.nicet")
    roomy = nice.TiledImage(t.width, t.height, t.channels, t.tile_w, t.tile_h,
                            torch.cat([t.packed, torch.full((80,), 0xA5, dtype=torch.uint8)]), t.off, t.stream_len, t.kind)
    nice.save_tiled(path, roomy)                      # only packed[:off[n]] is stored
    raw = open(path, "rb").read()
    n = 12
    assert len(raw) == HSZ + 8 * n + 8 * (n + 1) + 16 + t.nbytes      # 12 kinds padded to 16
    assert struct.unpack(HEADER, raw[:HSZ]) == (b"NICETILE", 1, 200, 136, 3, 64, 64, 4, 3, 0, t.nbytes)
    assert raw[HSZ + 8 * n + 8 * (n + 1):][:16] == bytes([0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    g = nice.load_tiled(path)
    assert (g.width, g.height, g.channels, g.tile_w, g.tile_h, g.nx, g.ny) == (200, 136, 3, 64, 64, 4, 3)
    assert g.packed.device.type == "cpu" and g.packed.dtype == torch.uint8 and g.kind.dtype == torch.uint8
    assert g.off.dtype == torch.int64 and g.stream_len.dtype == torch.int64
    assert torch.equal(g.packed, t.packed) and torch.equal(g.off, t.off)
    assert torch.equal(g.stream_len, t.stream_len) and torch.equal(g.kind, t.kind)
    _write(path, t)                                   # the hand-written file is the same file
    assert open(path, "rb").read() == raw

    def rejected(**kw):
        with pytest.raises(nice.NiceError) as e:
            nice.load_tiled(path)
        assert e.value.code == E_FORMAT, kw

    for cut in (len(raw) - 1, HSZ + 8 * n + 3, HSZ + 10, HSZ - 1, 0):   # blob, offsets, lengths, header, empty
        open(path, "wb").write(raw[:cut])
        rejected(cut=cut)
    open(path, "wb").write(raw + b"\0")
    rejected(extra=1)
    _write(path, t, magic=b"NICEPACK")
    rejected(magic=1)
    _write(path, t, version=2)
    rejected(version=2)
    kinds = t.kind.numpy().copy()
    kinds[2] = 2
    _write(path, t, kinds=kinds)
    rejected(kind=2)
    _write(path, t, kinds=np.concatenate([t.kind.numpy(), np.array([0, 0, 1, 0], np.uint8)]))   # a nonzero pad byte
    rejected(kind_pad=1)
    lens = t.stream_len.numpy().copy()
    lens[5] -= 1
    _write(path, t, lens=lens)                        # raw tile of the wrong length
    rejected(raw_len=1)
    kinds = t.kind.numpy().copy()
    kinds[1] = 1
    _write(path, t, kinds=kinds)                      # a coded tile's length called raw
    rejected(raw_len=2)
    _write(path, t, nx=3, ny=4)                       # 12 tiles, but not this image's grid
    rejected(grid=1)
    _write(path, t, tile_w=128)                       # grid and tile size disagree
    rejected(grid=2)
    _write(path, t, width=300)
    rejected(grid=3)
    _write(path, t, tile_w=1, nx=200)
    rejected(tile=1)
    _write(path, t, channels=5)
    rejected(channels=5)
    offs = t.off.numpy().copy()
    offs[3] += 8
    _write(path, t, offs=offs)                        # not 16-byte aligned
    rejected(aligned=1)
    offs = t.off.numpy().copy()
    offs[3], offs[4] = offs[4], offs[3]
    _write(path, t, offs=offs)                        # not monotone
    rejected(monotone=1)
    lens = t.stream_len.numpy().copy()
    lens[0] = int(t.off[1]) + 1
    _write(path, t, lens=lens)                        # tile 0 runs into tile 1
    rejected(overlap=1)
    offs = t.off.numpy().copy()
    offs[-1] += 16
    _write(path, t, offs=offs)                        # off[n] != the packed size
    rejected(size=1)
    offs = t.off.numpy().copy()
    offs[0] = 16
    _write(path, t, offs=offs)
    rejected(first=1)
    _write(path, t, size=t.nbytes + 16, blob=t.packed.numpy().tobytes() + bytes(16))   # size and offsets disagree
    rejected(size=2)
