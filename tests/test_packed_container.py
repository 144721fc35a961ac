"""The host-side container of a packed batch (save_packed / load_packed): CPU
tensors only, no GPU and no libnice_hip.so."""
import struct

import numpy as np
import pytest

HEADER = "<8sIIIIIIQ"   # magic, version, n, width, height, channels, reserved, packed size
HSZ = struct.calcsize(HEADER)


def _fake_batch(torch, lens):
    """Fake streams in the packed layout: off[f + 1] = off[f] + align16(len[f]), pads zero."""
    rng = np.random.default_rng(11)
    lens = np.asarray(lens, np.int64)
    off = np.zeros(lens.size + 1, np.int64)
    np.cumsum((lens + 15) // 16 * 16, out=off[1:])
    blob = np.zeros(int(off[-1]), np.uint8)
    for f, l in enumerate(lens):
        blob[off[f]:off[f] + l] = rng.integers(1, 256, l, dtype=np.uint8)
    return torch.from_numpy(blob), torch.from_numpy(off), torch.from_numpy(lens)


def _write(path, n, lens, offs, blob, magic=b"NICEPACK", version=1, size=None):
    with open(path, "wb") as fh:
        fh.write(struct.pack(HEADER, magic, version, n, 64, 48, 4, 0, len(blob) if size is None else size))
        fh.write(np.asarray(lens, "<u8").tobytes())
        fh.write(np.asarray(offs, "<u8").tobytes())
        fh.write(bytes(blob))


def test_container_round_trip_and_rejects(nice, tmp_path):
    import torch
    loaded_before = nice._lib   # (another test may have loaded the library; this one must not)
    packed, off, lens = _fake_batch(torch, [0, 1, 15, 16, 17, 1000, 0, 4097])
    path = str(tmp_path / "batch.nicepack")
    # a buffer larger than off[n]: only packed[:off[n]] is stored
    roomy = torch.cat([packed, torch.full((80,), 0xA5, dtype=torch.uint8)])
    nice.save_packed(path, roomy, off, lens, 640, 360, 4)
    raw = open(path, "rb").read()
    n = lens.numel()
    assert len(raw) == HSZ + 8 * n + 8 * (n + 1) + int(off[n])
    assert struct.unpack(HEADER, raw[:HSZ]) == (b"NICEPACK", 1, n, 640, 360, 4, 0, int(off[n]))
    p2, o2, l2, w, h, c = nice.load_packed(path)
    assert (w, h, c) == (640, 360, 4)
    assert p2.device.type == "cpu" and p2.dtype == torch.uint8 and o2.dtype == torch.int64 and l2.dtype == torch.int64
    assert torch.equal(p2, packed) and torch.equal(o2, off) and torch.equal(l2, lens)
    # an empty batch is a valid file
    nice.save_packed(path, torch.zeros(0, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64),
                     torch.zeros(0, dtype=torch.int64), 1, 1, 3)
    p0, o0, l0, *_ = nice.load_packed(path)
    assert p0.numel() == 0 and o0.tolist() == [0] and l0.numel() == 0

    def rejected(**kw):
        with pytest.raises(nice.NiceError) as e:
            nice.load_packed(path)
        assert e.value.code == nice.E_FORMAT, kw

    good_l, good_o, blob = [5, 20, 16], [0, 16, 48, 64], bytes(range(64))
    _write(path, 3, good_l, good_o, blob)
    assert nice.load_packed(path)[1].tolist() == good_o
    for cut in (len(raw) - 1, HSZ + 10, HSZ - 1, 0):   # truncated: blob, tables, header, empty
        open(path, "wb").write(raw[:cut])
        rejected(cut=cut)
    open(path, "wb").write(raw + b"\0")                 # trailing bytes
    rejected(extra=1)
    _write(path, 3, good_l, good_o, blob, magic=b"NICEPUCK")
    rejected(magic=1)
    _write(path, 3, good_l, good_o, blob, version=2)
    rejected(version=2)
    _write(path, 3, good_l, [0, 48, 16, 64], blob)      # not monotone
    rejected(monotone=1)
    _write(path, 3, good_l, [0, 8, 48, 64], blob)       # not 16-byte aligned
    rejected(aligned=1)
    _write(path, 3, [5, 33, 16], good_o, blob)          # off[1] + len[1] > off[2]
    rejected(overlap=1)
    _write(path, 3, good_l, [0, 16, 48, 80], blob)      # off[n] != the packed size
    rejected(size=1)
    _write(path, 3, good_l, [16, 16, 48, 64], blob)     # off[0] != 0
    rejected(first=1)
    assert nice._lib is loaded_before                   # nothing here loaded libnice_hip.so
