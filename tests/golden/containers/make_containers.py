#!/usr/bin/env python3
"""Regenerate the golden container files in this directory.

Five files written by save_packed / save_tiled / save_set from fixed CPU
tensors (no GPU and no library call): a NICEPACK, a NICETILE version 1 and
version 2, a NICESETS version 1 and version 2.  They pin the bytes of every
table a container holds; tests/test_container_golden.py rebuilds the same
tensors with ``cases`` and asserts that save_* still writes these bytes and
that load_* returns the tensors.

The geometry is the smallest that exercises every table: a 5 x 3 image at
2 x 2 tiles (3 x 2 tiles: six kinds padded to eight bytes, a raw tile of 12
bytes), a set of that image and a 2 x 2 one (seven tiles), and an alpha batch
with coded, raw (4 bytes) and constant tiles.  The streams are fake bytes.

    python tests/golden/containers/make_containers.py          # rewrite the files
    python tests/golden/containers/make_containers.py --check  # verify, exit 1 on mismatch
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
TW, TH = 2, 2


def _batch(torch, rng, lens):
    """(packed, off, stream_len) of fake streams of ``lens`` bytes, 16-byte aligned."""
    lens = np.asarray(lens, np.int64)
    off = np.zeros(lens.size + 1, np.int64)
    np.cumsum((lens + 15) // 16 * 16, out=off[1:])
    blob = np.zeros(int(off[-1]), np.uint8)
    for t in range(lens.size):
        blob[off[t]:off[t] + lens[t]] = rng.integers(1, 256, lens[t], dtype=np.uint8)
    return torch.from_numpy(blob), torch.from_numpy(off), torch.from_numpy(lens)


def _alpha(torch, nice, rng, n):
    """An alpha batch over n tiles: tile 1 raw, tiles 2 and n - 1 constant, the rest coded."""
    lens, kind, val = rng.integers(5, 40, n), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    lens[1], kind[1] = TW * TH, 1
    for t, v in ((2, 255), (n - 1, 7)):
        lens[t], kind[t], val[t] = 0, 2, v
    return nice.TiledAlpha(*_batch(torch, rng, lens), torch.from_numpy(kind), torch.from_numpy(val))


def cases(nice, torch):
    """{file name: (save, load, object)}; ``save(path, object)`` writes the file."""
    rng = np.random.default_rng(20261020)
    out = {}
    packed = _batch(torch, rng, [33, 16, 1])
    out["batch.nicepack"] = (lambda path, o: nice.save_packed(path, *o), nice.load_packed, packed + (7, 5, 3))
    for name, alpha in (("image_v1.nicetile", False), ("image_v2.nicetile", True)):
        lens, kind = rng.integers(5, 60, 6), np.zeros(6, np.uint8)
        lens[4], kind[4] = TW * TH * 3, 1
        t = nice.TiledImage(5, 3, 4 if alpha else 3, TW, TH, *_batch(torch, rng, lens), torch.from_numpy(kind))
        if alpha:
            t.alpha = _alpha(torch, nice, rng, 6)
        out[name] = (nice.save_tiled, nice.load_tiled, t)
    for name, alpha in (("set_v1.nicesets", False), ("set_v2.nicesets", True)):
        lens, kind = rng.integers(5, 60, 7), np.zeros(7, np.uint8)
        for t in (0, 6):
            lens[t], kind[t] = TW * TH * 3, 1
        s = nice.ImageSet([5, 2], [3, 2], 4 if alpha else 3, TW, TH, [0, 6, 7], *_batch(torch, rng, lens),
                          torch.from_numpy(kind))
        if alpha:
            s.alpha = _alpha(torch, nice, rng, 7)
        out[name] = (nice.save_set, nice.load_set, s)
    return out


def main(check):
    import tempfile
    import torch
    sys.path.insert(0, ROOT)
    nice = importlib.import_module("fast-losless-image-compression-format_amd")
    bad = 0
    for name, (save, _, obj) in cases(nice, torch).items():
        path = os.path.join(HERE, name)
        if check:
            with tempfile.TemporaryDirectory() as tmp:
                save(os.path.join(tmp, name), obj)
                ok = open(os.path.join(tmp, name), "rb").read() == open(path, "rb").read()
            print(("ok  " if ok else "BAD ") + name)
            bad += not ok
        else:
            save(path, obj)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main("--check" in sys.argv))
