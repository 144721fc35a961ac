"""The NICESETS container with an alpha batch (version 2) without a GPU or the
library: round trip from hand-made tables on CPU tensors, the version 1 file of
a set without alpha byte for byte as before, and one rejection for every check
the version 2 loader makes that the version 1 loader does not."""
import dataclasses
import struct

import numpy as np
import pytest

from test_sets_container import HEADER, HSZ, _fake, _write

E_ARG, E_FORMAT = -1, -5


def _fake_alpha(torch, nice):
    """A 4-channel ImageSet of fake streams with a fake alpha batch: coded,
    raw (tiles 7 and 40) and constant (every third tile) entries."""
    s = dataclasses.replace(_fake(torch, nice), channels=4)
    n = s.first[-1]
    rng = np.random.default_rng(9)
    kind = np.zeros(n, np.uint8)
    kind[::3] = 2
    kind[[7, 40]] = 1
    lens = rng.integers(20, 900, n).astype(np.int64)
    lens[kind == 2] = 0
    lens[kind == 1] = s.tile_w * s.tile_h
    val = np.where(kind == 2, rng.integers(0, 256, n), 0).astype(np.uint8)
    off = np.zeros(n + 1, np.int64)
    np.cumsum((lens + 15) // 16 * 16, out=off[1:])
    blob = np.zeros(int(off[-1]), np.uint8)
    for t in range(n):
        blob[off[t]:off[t] + lens[t]] = rng.integers(1, 256, lens[t], dtype=np.uint8)
    s.alpha = nice.TiledAlpha(torch.from_numpy(blob), torch.from_numpy(off), torch.from_numpy(lens),
                              torch.from_numpy(kind), torch.from_numpy(val))
    return s


def _pad8(b):
    return b + bytes(-len(b) % 8)


def _write2(path, s, tail=b"", **kw):
    """The version 2 container written out by hand: test_sets_container's
    colour part with version 2 and flags 1, then the alpha part, any field
    replaced through kw (those of _write, and asize, alens, aoffs, akinds,
    avals, ablob)."""
    a = s.alpha
    n = s.first[-1]
    f = dict(asize=int(a.off[n]), alens=a.stream_len.numpy(), aoffs=a.off.numpy(), akinds=a.kind.numpy(),
             avals=a.value.numpy(), ablob=a.packed.numpy().tobytes())
    colour = dict(version=2, reserved=1)
    for k, v in kw.items():
        (f if k in f else colour)[k] = v
    _write(path, s, **colour)
    with open(path, "ab") as fh:
        fh.write(struct.pack("<Q", f["asize"]))
        fh.write(np.asarray(f["alens"], "<u8").tobytes())
        fh.write(np.asarray(f["aoffs"], "<u8").tobytes())
        fh.write(_pad8(np.asarray(f["akinds"], np.uint8).tobytes()))
        fh.write(_pad8(np.asarray(f["avals"], np.uint8).tobytes()))
        fh.write(f["ablob"])
        fh.write(tail)


def test_v2_round_trip_and_v1_unchanged(nice, tmp_path):
    import torch
    s = _fake_alpha(torch, nice)
    a = s.alpha
    n, K = 46, 6
    path = str(tmp_path / "set.nices")
    roomy = dataclasses.replace(a, packed=torch.cat([a.packed, torch.full((48,), 0xA5, dtype=torch.uint8)]))
    nice.save_set(path, dataclasses.replace(s, alpha=roomy))           # only packed[:off[n]] is stored
    raw = open(path, "rb").read()
    colour_end = HSZ + 8 * K + 8 * n + 8 * (n + 1) + 48 + s.nbytes
    assert len(raw) == colour_end + 8 + 8 * n + 8 * (n + 1) + 48 + 48 + a.nbytes      # 46 kinds, values padded to 48
    assert struct.unpack(HEADER, raw[:HSZ]) == (b"NICESETS", 2, 4, 64, 64, K, 1, n, s.nbytes)
    assert struct.unpack("<Q", raw[colour_end:colour_end + 8]) == (a.nbytes,)
    _write2(path, s)                                                   # the hand-written file is the same file
    assert open(path, "rb").read() == raw
    g = nice.load_set(path)
    assert (g.widths, g.heights, g.channels, g.tile_w, g.tile_h, g.first) == (s.widths, s.heights, 4, 64, 64, s.first)
    assert torch.equal(g.packed, s.packed) and torch.equal(g.off, s.off) and torch.equal(g.kind, s.kind)
    b = g.alpha
    assert b.packed.device.type == "cpu" and b.packed.dtype == torch.uint8
    assert b.off.dtype == torch.int64 and b.stream_len.dtype == torch.int64
    assert b.kind.dtype == torch.uint8 and b.value.dtype == torch.uint8
    assert torch.equal(b.packed, a.packed) and torch.equal(b.off, a.off) and torch.equal(b.stream_len, a.stream_len)
    assert torch.equal(b.kind, a.kind) and torch.equal(b.value, a.value)
    # without alpha: version 1, byte for byte the layout of test_sets_container's hand-written file
    plain = dataclasses.replace(s, alpha=None)
    nice.save_set(path, plain)
    v1 = open(path, "rb").read()
    assert v1 == raw[:8] + struct.pack("<I", 1) + raw[12:28] + struct.pack("<I", 0) + raw[32:colour_end]
    _write(path, plain)
    assert open(path, "rb").read() == v1
    assert nice.load_set(path).alpha is None
    # positional construction without the new field still works, and save_set refuses alpha on 3 channels
    old = nice.ImageSet(s.widths, s.heights, 3, 64, 64, s.first, s.packed, s.off, s.stream_len, s.kind)
    assert old.alpha is None
    with pytest.raises(nice.NiceError) as e:
        nice.save_set(path, dataclasses.replace(old, alpha=a))
    assert e.value.code == E_ARG
    with pytest.raises(nice.NiceError) as e:
        nice.save_set(path, dataclasses.replace(s, alpha=dataclasses.replace(a, kind=a.kind[:-1])))
    assert e.value.code == E_ARG


def test_v2_rejects(nice, tmp_path):
    import torch
    s = _fake_alpha(torch, nice)
    a = s.alpha
    n = 46
    path = str(tmp_path / "set.nices")
    _write2(path, s)
    raw = open(path, "rb").read()
    assert nice.load_set(path).alpha is not None
    colour_end = len(raw) - (8 + 8 * n + 8 * (n + 1) + 48 + 48 + a.nbytes)

    def rejected(**kw):
        with pytest.raises(nice.NiceError) as e:
            nice.load_set(path)
        assert e.value.code == E_FORMAT, kw

    # truncation inside the alpha part: blob, values, kinds, offsets, lengths, the size word, none of it at all
    for cut in (len(raw) - 1, len(raw) - a.nbytes - 3, len(raw) - a.nbytes - 50, colour_end + 8 + 8 * n + 5,
                colour_end + 8 + 3, colour_end + 5, colour_end):
        open(path, "wb").write(raw[:cut])
        rejected(cut=cut)
    _write2(path, s, tail=b"\0")
    rejected(extra=1)
    _write2(path, s, tail=bytes(16))
    rejected(extra=16)
    for flags in (0, 3, 2):                           # version 2 always has the alpha flag, and no other
        _write2(path, s, reserved=flags)
        rejected(flags=flags)
    _write2(path, s, version=3)
    rejected(version=3)
    _write2(path, s, channels=3)
    rejected(channels=3)
    _write(path, s, version=1, reserved=0)            # the colour part alone is a good version 1 file ...
    assert nice.load_set(path).alpha is None
    _write2(path, s, version=1, reserved=0)           # ... which nothing may follow
    rejected(v1_with_alpha_part=1)
    _write2(path, s, asize=a.nbytes + 8, ablob=a.packed.numpy().tobytes() + bytes(8))
    rejected(asize=8)
    _write2(path, s, asize=a.nbytes + 16, ablob=a.packed.numpy().tobytes() + bytes(16))   # size and offsets disagree
    rejected(asize=16)
    _write2(path, s, asize=a.nbytes + 16)             # the file is shorter than the size says
    rejected(fsize=1)
    _write2(path, s, asize=2**62)
    rejected(asize=2**62)
    offs = a.off.numpy().copy()
    offs[3] += 8
    _write2(path, s, aoffs=offs)                      # not 16-byte aligned
    rejected(aligned=1)
    offs = a.off.numpy().copy()
    offs[4], offs[5] = offs[5], offs[4]
    _write2(path, s, aoffs=offs)                      # not monotone
    rejected(monotone=1)
    offs = a.off.numpy().copy()
    offs[0] = 16
    _write2(path, s, aoffs=offs)
    rejected(first=1)
    lens = a.stream_len.numpy().copy()
    lens[1] = int(a.off[2] - a.off[1]) + 1
    _write2(path, s, alens=lens)                      # tile 1 runs into tile 2
    rejected(overlap=1)
    kinds = a.kind.numpy().copy()
    kinds[1] = 3
    _write2(path, s, akinds=kinds)
    rejected(kind=3)
    _write2(path, s, akinds=np.concatenate([a.kind.numpy(), np.array([0, 1], np.uint8)]))   # a nonzero pad byte
    rejected(kind_pad=1)
    _write2(path, s, avals=np.concatenate([a.value.numpy(), np.array([1, 0], np.uint8)]))
    rejected(value_pad=1)
    lens = a.stream_len.numpy().copy()
    lens[40] -= 1
    _write2(path, s, alens=lens)                      # raw plane of the wrong length
    rejected(raw_len=1)
    kinds = a.kind.numpy().copy()
    kinds[1] = 1
    _write2(path, s, akinds=kinds)                    # a coded tile's length called raw
    rejected(raw_len=2)
    kinds = a.kind.numpy().copy()
    kinds[1] = 2
    _write2(path, s, akinds=kinds)                    # a constant tile with a length
    rejected(const_len=1)
    vals = a.value.numpy().copy()
    vals[1] = 9
    _write2(path, s, avals=vals)                      # a value on a tile that is not constant
    rejected(value=1)
    _write2(path, s)
    assert nice.load_set(path).alpha is not None
