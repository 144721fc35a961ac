"""Image sets without a GPU: the set's tile scan and window selection of the C
ABI (nice_set_grid / nice_set_select) against brute force, and the NICESETS
container (save_set / load_set) on CPU tensors."""
import struct

import numpy as np
import pytest

HEADER = "<8sIIIIIIQQ"   # magic, version, channels, tile_w, tile_h, K, reserved, tile count, packed size
HSZ = struct.calcsize(HEADER)
E_ARG, E_FORMAT = -1, -5

# (widths, heights, tile_w, tile_h)
SETS = [([200, 333, 65, 5, 64, 130], [136, 211, 1, 7, 64, 70], 64, 64),
        ([200, 333, 65, 5, 64, 130], [136, 211, 1, 7, 64, 70], 66, 70),
        ([129], [70], 64, 35),                                           # K = 1
        ([9, 9, 2], [9, 1, 2], 2, 2)]


def _tiles_touched(w, h, tw, th, x0, y0, rw, rh):
    """Tile indices (row-major, ascending) of the pixels of a rectangle, pixel by pixel."""
    nx = -(-w // tw)
    lab = (np.arange(h) // th)[:, None] * nx + (np.arange(w) // tw)[None, :]
    return sorted(set(lab[y0:y0 + rh, x0:x0 + rw].reshape(-1).tolist()))


@pytest.mark.parametrize("ws,hs,tw,th", SETS)
def test_set_grid_matches_brute_force(nice, ws, hs, tw, th):
    first = nice.set_grid(ws, hs, tw, th)
    want = [0]
    for w, h in zip(ws, hs):
        want.append(want[-1] + len(_tiles_touched(w, h, tw, th, 0, 0, w, h)))
    assert first == want
    assert nice.set_bound(ws, hs, tw, th) == nice.packed_bound(want[-1], tw, th)
    if len(ws) == 1:
        nx, ny = nice.tile_grid(ws[0], hs[0], tw, th)
        assert first == [0, nx * ny]


def _refused(nice, fn, *a):
    with pytest.raises(nice.NiceError) as e:
        fn(*a)
    assert e.value.code == E_ARG, a


def test_set_grid_rejects(nice):
    _refused(nice, nice.set_grid, [], [], 64, 64)                       # K = 0
    _refused(nice, nice.set_grid, [200, 0], [136, 10], 64, 64)          # a zero width
    _refused(nice, nice.set_grid, [200, 10], [136, 0], 64, 64)
    _refused(nice, nice.set_grid, [200], [136], 1, 64)
    _refused(nice, nice.set_grid, [200], [136], 64, 8193)
    _refused(nice, nice.set_grid, [200, 32768], [136, 32769], 64, 64)   # one image above 2^30 pixels
    assert nice.set_bound([200, 0], [136, 10], 64, 64) == 0
    # 2^28 tiles of one encoder tile each per image: 15 images fit the 32-bit work counter, 16 do not
    assert nice.set_grid([32768] * 15, [32768] * 15, 2, 2)[-1] == 15 << 28
    _refused(nice, nice.set_grid, [32768] * 16, [32768] * 16, 2, 2)


def test_set_select_matches_brute_force(nice):
    ws, hs, tw, th = SETS[0]
    windows = [(1, 10, 10, 300, 190), (1, 60, 60, 10, 10),      # two windows on one image, the second across a corner
               (0, 70, 70, 20, 30),                             # inside one tile
               (3, 0, 0, 5, 7), (2, 0, 0, 65, 1),               # equal to their images
               (5, 63, 63, 2, 2), (4, 0, 0, 64, 64), (0, 199, 135, 1, 1)]
    sf = nice.set_select(ws, hs, tw, th, windows)
    want = [0]
    for i, x0, y0, rw, rh in windows:
        touched = _tiles_touched(ws[i], hs[i], tw, th, x0, y0, rw, rh)
        tx0, ty0, tx1, ty1 = nice.tile_select(ws[i], hs[i], tw, th, x0, y0, rw, rh)
        nx = -(-ws[i] // tw)
        assert [ty * nx + tx for ty in range(ty0, ty1) for tx in range(tx0, tx1)] == touched
        want.append(want[-1] + len(touched))
    assert sf == want and sf[1] - sf[0] == 20 and sf[2] - sf[1] == 4 and sf[3] - sf[2] == 1
    _refused(nice, nice.set_select, ws, hs, tw, th, [(6, 0, 0, 1, 1)])          # image index K
    _refused(nice, nice.set_select, ws, hs, tw, th, [(0, 0, 0, 0, 5)])          # empty
    _refused(nice, nice.set_select, ws, hs, tw, th, [(0, 0, 0, 5, 0)])
    _refused(nice, nice.set_select, ws, hs, tw, th, [(0, 0, 0, 1, 1), (3, 4, 0, 2, 1)])   # past the right edge of 5 x 7
    _refused(nice, nice.set_select, ws, hs, tw, th, [(2, 0, 0, 65, 2)])         # past the bottom edge of 65 x 1
    _refused(nice, nice.set_select, ws, hs, tw, th, [(0, 2**32 - 1, 0, 2, 1)])
    _refused(nice, nice.set_select, ws, hs, 1, th, [(0, 0, 0, 1, 1)])


def _fake(torch, nice, raw=(5, 40)):
    """An ImageSet of fake streams in the packed layout, two tiles raw."""
    ws, hs, tw, th = SETS[0]
    rng = np.random.default_rng(3)
    first = [0, 12, 36, 38, 39, 40, 46]
    n = first[-1]
    lens = rng.integers(20, 900, n).astype(np.int64)
    kind = np.zeros(n, np.uint8)
    for t in raw:
        lens[t], kind[t] = tw * th * 3, 1
    off = np.zeros(n + 1, np.int64)
    np.cumsum((lens + 15) // 16 * 16, out=off[1:])
    blob = np.zeros(int(off[-1]), np.uint8)
    for t in range(n):
        blob[off[t]:off[t] + lens[t]] = rng.integers(1, 256, lens[t], dtype=np.uint8)
    return nice.ImageSet(list(ws), list(hs), 3, tw, th, first, torch.from_numpy(blob), torch.from_numpy(off),
                         torch.from_numpy(lens), torch.from_numpy(kind))


def _write(path, s, **kw):
    """The container written out by hand, any field replaced through kw."""
    n = s.first[-1]
    f = dict(magic=b"NICESETS", version=1, channels=s.channels, tile_w=s.tile_w, tile_h=s.tile_h, K=len(s.widths),
             reserved=0, n=n, size=int(s.off[n]), widths=s.widths, heights=s.heights, lens=s.stream_len.numpy(),
             offs=s.off.numpy(), kinds=s.kind.numpy(), blob=s.packed.numpy().tobytes())
    f.update(kw)
    with open(path, "wb") as fh:
        fh.write(struct.pack(HEADER, f["magic"], f["version"], f["channels"], f["tile_w"], f["tile_h"], f["K"],
                             f["reserved"], f["n"], f["size"]))
        for w, h in zip(f["widths"], f["heights"]):
            fh.write(struct.pack("<II", w, h))
        fh.write(np.asarray(f["lens"], "<u8").tobytes())
        fh.write(np.asarray(f["offs"], "<u8").tobytes())
        k = np.asarray(f["kinds"], np.uint8).tobytes()
        fh.write(k + bytes(-len(k) % 8))
        fh.write(f["blob"])


def test_container_round_trip_and_rejects(nice, tmp_path):
    import dataclasses
    import torch
    s = _fake(torch, nice)
    n, K = 46, 6
    assert s.nbytes == int(s.off[n]) and len(s) == K
    path = str(tmp_path / "set.nices")
    roomy = dataclasses.replace(s, packed=torch.cat([s.packed, torch.full((80,), 0xA5, dtype=torch.uint8)]))
    nice.save_set(path, roomy)                        # only packed[:off[n]] is stored
    raw = open(path, "rb").read()
    assert HSZ == 48 and len(raw) == HSZ + 8 * K + 8 * n + 8 * (n + 1) + 48 + s.nbytes      # 46 kinds padded to 48
    assert struct.unpack(HEADER, raw[:HSZ]) == (b"NICESETS", 1, 3, 64, 64, K, 0, n, s.nbytes)
    assert struct.unpack("<12I", raw[HSZ:HSZ + 48]) == (200, 136, 333, 211, 65, 1, 5, 7, 64, 64, 130, 70)
    g = nice.load_set(path)
    assert (g.widths, g.heights, g.channels, g.tile_w, g.tile_h, g.first) == (s.widths, s.heights, 3, 64, 64, s.first)
    assert g.packed.device.type == "cpu" and g.packed.dtype == torch.uint8 and g.kind.dtype == torch.uint8
    assert g.off.dtype == torch.int64 and g.stream_len.dtype == torch.int64
    assert torch.equal(g.packed, s.packed) and torch.equal(g.off, s.off)
    assert torch.equal(g.stream_len, s.stream_len) and torch.equal(g.kind, s.kind)
    _write(path, s)                                   # the hand-written file is the same file
    assert open(path, "rb").read() == raw

    def rejected(**kw):
        with pytest.raises(nice.NiceError) as e:
            nice.load_set(path)
        assert e.value.code == E_FORMAT, kw

    for cut in (len(raw) - 1, HSZ + 8 * K + 8 * n + 3, HSZ + 8 * K + 10, HSZ + 5, HSZ - 1, 0):
        open(path, "wb").write(raw[:cut])             # blob, offsets, lengths, sizes, header, empty
        rejected(cut=cut)
    open(path, "wb").write(raw + b"\0")
    rejected(extra=1)
    _write(path, s, magic=b"NICETILE")
    rejected(magic=1)
    _write(path, s, version=2)
    rejected(version=2)
    _write(path, s, reserved=1)
    rejected(reserved=1)
    _write(path, s, channels=5)
    rejected(channels=5)
    _write(path, s, tile_w=1)
    rejected(tile=1)
    _write(path, s, tile_w=128)                       # the sizes give another tile count at this tile size
    rejected(tile=2)
    _write(path, s, K=5)                              # one image fewer than the file holds
    rejected(K=5)
    _write(path, s, K=0)
    rejected(K=0)
    _write(path, s, K=2**32 - 1)
    rejected(K=-1)
    _write(path, s, widths=[200, 333, 65, 5, 65, 130])   # 64 -> 65 pixels: one tile more than n
    rejected(size_of_image=1)
    _write(path, s, widths=[200, 333, 65, 0, 64, 130])
    rejected(size_of_image=0)
    _write(path, s, n=n + 1)
    rejected(n=1)
    _write(path, s, n=2**40)
    rejected(n=2)
    _write(path, s, size=s.nbytes + 16, blob=s.packed.numpy().tobytes() + bytes(16))   # size and offsets disagree
    rejected(size=2)
    _write(path, s, size=s.nbytes + 8, blob=s.packed.numpy().tobytes() + bytes(8))
    rejected(size=3)
    offs = s.off.numpy().copy()
    offs[3] += 8
    _write(path, s, offs=offs)                        # not 16-byte aligned
    rejected(aligned=1)
    offs = s.off.numpy().copy()
    offs[3], offs[4] = offs[4], offs[3]
    _write(path, s, offs=offs)                        # not monotone
    rejected(monotone=1)
    offs = s.off.numpy().copy()
    offs[0] = 16
    _write(path, s, offs=offs)
    rejected(first=1)
    lens = s.stream_len.numpy().copy()
    lens[0] = int(s.off[1]) + 1
    _write(path, s, lens=lens)                        # tile 0 runs into tile 1
    rejected(overlap=1)
    kinds = s.kind.numpy().copy()
    kinds[2] = 2
    _write(path, s, kinds=kinds)
    rejected(kind=2)
    _write(path, s, kinds=np.concatenate([s.kind.numpy(), np.array([0, 1], np.uint8)]))   # a nonzero pad byte
    rejected(kind_pad=1)
    lens = s.stream_len.numpy().copy()
    lens[40] -= 1
    _write(path, s, lens=lens)                        # raw tile of the wrong length
    rejected(raw_len=1)
    kinds = s.kind.numpy().copy()
    kinds[1] = 1
    _write(path, s, kinds=kinds)                      # a coded tile's length called raw
    rejected(raw_len=2)
    _write(path, s)
    assert nice.load_set(path).first == s.first
