"""The NICETILE container with an alpha batch, without a GPU: version 2 round
trip on CPU tensors, version 1 files unchanged byte for byte, and every
malformed alpha table refused (save_tiled / load_tiled)."""
import dataclasses
import struct

import numpy as np
import pytest

HEADER = "<8sIIIIIIIIIQ"   # magic, version, width, height, channels, tile_w, tile_h, nx, ny, reserved / flags, packed size
HSZ = struct.calcsize(HEADER)
E_FORMAT = -5
W, H, TW, TH, N = 200, 136, 64, 64, 12


def _packed(rng, lens):
    off = np.zeros(lens.size + 1, np.int64)
    np.cumsum((lens + 15) // 16 * 16, out=off[1:])
    blob = np.zeros(int(off[-1]), np.uint8)
    for t in range(lens.size):
        blob[off[t]:off[t] + lens[t]] = rng.integers(1, 256, lens[t], dtype=np.uint8)
    return off, blob


def _fake(torch, nice, alpha=True):
    """A 4 x 3 RGBA TiledImage of fake streams, colour tile 5 raw; its alpha
    batch has coded, raw (tiles 2, 7) and constant (0, 1, 9, 11) tiles."""
    rng = np.random.default_rng(7)
    lens = rng.integers(20, 900, N).astype(np.int64)
    kind = np.zeros(N, np.uint8)
    lens[5], kind[5] = TW * TH * 3, 1
    off, blob = _packed(rng, lens)
    t = nice.TiledImage(W, H, 4, TW, TH, torch.from_numpy(blob), torch.from_numpy(off), torch.from_numpy(lens),
                        torch.from_numpy(kind))
    if alpha:
        alens = rng.integers(14, 500, N).astype(np.int64)
        akind = np.zeros(N, np.uint8)
        aval = np.zeros(N, np.uint8)
        for i in (2, 7):
            alens[i], akind[i] = TW * TH, 1
        for i, v in ((0, 255), (1, 0), (9, 17), (11, 255)):
            alens[i], akind[i], aval[i] = 0, 2, v
        aoff, ablob = _packed(rng, alens)
        t.alpha = nice.TiledAlpha(torch.from_numpy(ablob), torch.from_numpy(aoff), torch.from_numpy(alens),
                                  torch.from_numpy(akind), torch.from_numpy(aval))
    return t


def _pad8(a):
    b = np.asarray(a, np.uint8).tobytes()
    return b + bytes(-len(b) % 8)


def _write(path, t, **kw):
    """The version 2 container written out by hand, any alpha field replaced through kw."""
    a = t.alpha
    f = dict(version=2, flags=1, channels=4, asize=int(a.off[N]), alens=a.stream_len.numpy(), aoffs=a.off.numpy(),
             akinds=_pad8(a.kind.numpy()), avals=_pad8(a.value.numpy()), ablob=a.packed.numpy().tobytes())
    f.update(kw)
    with open(path, "wb") as fh:
        fh.write(struct.pack(HEADER, b"NICETILE", f["version"], W, H, f["channels"], TW, TH, 4, 3, f["flags"],
                             int(t.off[N])))
        fh.write(np.asarray(t.stream_len.numpy(), "<u8").tobytes())
        fh.write(np.asarray(t.off.numpy(), "<u8").tobytes())
        fh.write(_pad8(t.kind.numpy()))
        fh.write(t.packed.numpy().tobytes())
        fh.write(struct.pack("<Q", f["asize"]))
        fh.write(np.asarray(f["alens"], "<u8").tobytes())
        fh.write(np.asarray(f["aoffs"], "<u8").tobytes())
        fh.write(f["akinds"])
        fh.write(f["avals"])
        fh.write(f["ablob"])


def test_alpha_container_round_trip(nice, tmp_path):
    import torch
    t = _fake(torch, nice)
    a = t.alpha
    assert a.nbytes == int(a.off[N]) == a.packed.numel()
    path = str(tmp_path / "img.nicet")
    roomy = dataclasses.replace(t, alpha=dataclasses.replace(
        a, packed=torch.cat([a.packed, torch.full((48,), 0xA5, dtype=torch.uint8)])))
    nice.save_tiled(path, roomy)                       # only alpha.packed[:off[n]] is stored
    raw = open(path, "rb").read()
    colour_end = HSZ + 8 * N + 8 * (N + 1) + 16 + t.nbytes
    assert len(raw) == colour_end + 8 + 8 * N + 8 * (N + 1) + 16 + 16 + a.nbytes
    assert struct.unpack(HEADER, raw[:HSZ]) == (b"NICETILE", 2, W, H, 4, TW, TH, 4, 3, 1, t.nbytes)
    assert struct.unpack("<Q", raw[colour_end:colour_end + 8]) == (a.nbytes,)
    _write(path, t)                                    # the hand-written file is the same file
    assert open(path, "rb").read() == raw
    g = nice.load_tiled(path)                          # device=None: no GPU, no library
    assert (g.width, g.height, g.channels, g.tile_w, g.tile_h) == (W, H, 4, TW, TH)
    assert torch.equal(g.packed, t.packed) and torch.equal(g.off, t.off)
    assert torch.equal(g.stream_len, t.stream_len) and torch.equal(g.kind, t.kind)
    ga = g.alpha
    assert ga is not None and ga.packed.device.type == "cpu" and ga.packed.dtype == torch.uint8
    assert ga.off.dtype == torch.int64 and ga.stream_len.dtype == torch.int64
    assert ga.kind.dtype == torch.uint8 and ga.value.dtype == torch.uint8
    assert torch.equal(ga.packed, a.packed) and torch.equal(ga.off, a.off) and torch.equal(ga.stream_len, a.stream_len)
    assert torch.equal(ga.kind, a.kind) and torch.equal(ga.value, a.value)
    assert ga.kind.tolist() == [2, 2, 1, 0, 0, 0, 0, 1, 0, 2, 0, 2] and ga.value.tolist()[9] == 17


def test_version_1_is_unchanged(nice, tmp_path):
    """Without alpha the file is version 1, byte for byte the hand-packed one,
    and loads with alpha None."""
    import torch
    t = _fake(torch, nice, alpha=False)
    assert t.alpha is None
    path = str(tmp_path / "v1.nicet")
    nice.save_tiled(path, t)
    want = (struct.pack(HEADER, b"NICETILE", 1, W, H, 4, TW, TH, 4, 3, 0, t.nbytes)
            + np.asarray(t.stream_len.numpy(), "<u8").tobytes() + np.asarray(t.off.numpy(), "<u8").tobytes()
            + _pad8(t.kind.numpy()) + t.packed.numpy().tobytes())
    assert open(path, "rb").read() == want
    g = nice.load_tiled(path)
    assert g.alpha is None and torch.equal(g.packed, t.packed) and torch.equal(g.kind, t.kind)


def test_malformed_alpha_tables_are_refused(nice, tmp_path):
    import torch
    t = _fake(torch, nice)
    a = t.alpha
    path = str(tmp_path / "bad.nicet")
    _write(path, t)
    assert nice.load_tiled(path).alpha is not None     # (the unmodified file loads)
    raw = open(path, "rb").read()

    def rejected(**kw):
        if kw:
            _write(path, t, **kw)
        with pytest.raises(nice.NiceError) as e:
            nice.load_tiled(path)
        assert e.value.code == E_FORMAT, list(kw)

    def tab(name, **put):
        v = getattr(a, name).numpy().copy()
        for i, x in put.items():
            v[int(i[1:])] = x
        return v

    colour_end = HSZ + 8 * N + 8 * (N + 1) + 16 + t.nbytes
    for cut in (len(raw) - 1, colour_end + 8 + 8 * N + 3, colour_end + 4, colour_end):   # blob, offsets, size, no alpha part
        open(path, "wb").write(raw[:cut])
        rejected()
    open(path, "wb").write(raw + b"\0")                 # exact file size
    rejected()
    rejected(flags=0)                                   # version 2 says alpha
    rejected(flags=3)
    rejected(version=1)                                 # version 1 has no flags and no alpha part
    rejected(version=3)
    rejected(channels=3)
    offs = tab("off")
    offs[3] += 8
    rejected(aoffs=offs)                                # not 16-byte aligned
    offs = tab("off")
    offs[4], offs[5] = offs[5], offs[4]
    rejected(aoffs=offs)                                # not monotone
    offs = tab("off")
    offs[0] = 16
    rejected(aoffs=offs)                                # not from 0
    offs = tab("off")
    offs[-1] += 16
    rejected(aoffs=offs)                                # not to the size
    rejected(asize=a.nbytes + 16, ablob=a.packed.numpy().tobytes() + bytes(16))   # size and offsets disagree
    rejected(asize=a.nbytes + 8, ablob=a.packed.numpy().tobytes() + bytes(8))     # size not a multiple of 16
    rejected(alens=tab("stream_len", t3=int(a.off[4] - a.off[3]) + 1))            # tile 3 runs into tile 4
    rejected(akinds=_pad8(tab("kind", t3=3)))           # a kind above 2
    rejected(akinds=_pad8(tab("kind"))[:12] + b"\0\1\0\0")                         # a nonzero pad byte
    rejected(avals=_pad8(tab("value"))[:12] + b"\0\0\1\0")
    rejected(alens=tab("stream_len", t2=TW * TH - 1))   # raw length
    rejected(akinds=_pad8(tab("kind", t3=1)))           # a coded tile's length called raw
    rejected(akinds=_pad8(tab("kind", t3=2)))           # constant with a nonzero length
    rejected(avals=_pad8(tab("value", t3=9)))           # a value on a coded tile
    rejected(avals=_pad8(tab("value", t7=1)))           # a value on a raw tile
