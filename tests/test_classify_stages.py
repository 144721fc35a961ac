"""The stages the classify kernels share (the cls_* functions of
csrc/nice_classify.hip: work range, histogram flush on a frame change, ring
prefill and put, coded flags out, tile edges, in-tile run digits, the bounded
window load), through every kernel that has them: slide, pair, ring, ring2,
strip, twin (and the window kernel, which shares none, as the yardstick) --
as frames, where the coded flags go out and enc_rundigits counts the run
digits, as batches whose blocks cross frame boundaries, and as bands, where
the kernels count the run digits themselves.

One input for all of them: NICE-SYN-v1 with spans of one colour written over
linear pixel ranges, so that every image holds runs of 1, 2, 3 and 4 base-8
digits, a run starting at lane 63 of a wave, one across a wave boundary, one
across in-tile offset 511 -> 512 (found through the tile mask, not the wave's
ballot), one ending on a tile's last pixel, one crossing a tile end
(enc_tailruns') and one running to the frame's last pixel; the oracle's
histogram must show all eight run-digit prefixes.

Each case asserts the oracle's bytes, the kernel the library reports, and
that it is the one the planner gives (so an option that stops forcing its
kernel fails here instead of testing another one)."""
import functools
import importlib

import numpy as np
import pytest

import plan_driver
from test_classify_routes import PAIR, RING, RING2, SLIDE, STRIP, TWIN, WINDOW, _last, _same

pytestmark = pytest.mark.gpu

TILE = 1024
# (in-tile start, run length L: the coded pixel and L repeats of it), one tile each
SPANS = (
    ((100, 5), (200, 10), (300, 70)),   # L - 1 = 4, 9, 69: one, two, three base-8 digits
    ((50, 600),),                       # L - 1 = 599: four digits
    ((127, 4), (250, 7)),               # from lane 63 of a wave (digit 3); across pixels 255 | 256 (digit 6)
    ((505, 20),),                       # across 511 | 512: the next coded pixel is in the other half's mask words
    ((1000, 23),),                      # ends on the tile's last pixel
    ((1010, 30),),                      # crosses the tile's end: enc_tailruns'
)


@functools.lru_cache(maxsize=None)
def _run_input(w, h, c, seed):
    """(pixels, the oracle's stream): SYN-v1 with the spans above in tiles 1..6
    and again from the middle tile on (both bands of two get them), and a run to
    the last pixel.  The pixels either side of a span differ from it."""
    from conftest import oracle_mod
    O = oracle_mod()
    n = w * h
    px = O.gen_syn_v1(w, h, c, seed).reshape(n, c).copy()
    tiles = (n + TILE - 1) // TILE
    spans = [(n - 12, 11)]
    for base in (0, tiles // 2):
        assert (base + len(SPANS) + 1) * TILE + 64 <= n - 12 and (base == 0 or base > len(SPANS)), (w, h)
        for k, tile_spans in enumerate(SPANS):
            spans += [((base + 1 + k) * TILE + s, L) for s, L in tile_spans]
    for k, (s, L) in enumerate(spans):
        colour = np.array([17 + 5 * k, 201 - 3 * k, 90 + k, 255][:c], dtype=np.uint8)
        px[s:s + L + 1] = colour
        for j in (s - 1, s + L + 1):
            if j < n:
                px[j] = colour
                px[j, 0] ^= 0x80
    px = px.reshape(-1)
    stream, st = O.encode(px, w, h, c, with_stats=True)
    digits = [int(st.hist[256 + 5 + d]) for d in range(8)]   # BIN_PREFIX + P_RUN1 + d (csrc/nice_format.h)
    assert all(digits), (w, h, c, digits)
    return px, stream


def _options(opts, options):
    for name in options:
        opts.setenv(name, 1)
    return {name[len("NICE_ENC_"):].lower(): 1 for name in options}


def _encode(nice, frames, w, h, c, ctx):
    """frames: pixel arrays, encoded as one batch at a 16-byte aligned stride;
    (streams, (4-byte aligned, 16-byte aligned))."""
    import torch
    n = len(frames)
    stride = (w * h * c + 15) // 16 * 16
    t = torch.zeros((n, stride), dtype=torch.uint8)
    for i, f in enumerate(frames):
        t[i, :w * h * c] = torch.from_numpy(f)
    t = t.cuda()
    bound = (nice.encode_bound(w, h) + 255) // 256 * 256
    out = torch.zeros((n, bound), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    nice.encode_batch(t, w, h, c, out, lens, ctx=ctx)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return [bytes(o[i, :int(lens[i])]) for i in range(n)], [t.data_ptr() % a == 0 for a in (4, 16)]


def _check_frames(nice, opts, shape, n, kind, options):
    import torch
    w, h, c = shape
    plan_opts = _options(opts, options)
    inputs = [_run_input(w, h, c, 40 + i) for i in range(n)]
    ctx = nice.Context(0)
    got, (al4, al16) = _encode(nice, [px for px, _ in inputs], w, h, c, ctx)
    assert _last(nice, ctx) == kind
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert plan_driver.enc_plan(w, h, c, n, cus, al4=al4, al16=al16, **plan_opts)["kind_id"] == kind
    for i in range(n):
        _same(got[i], inputs[i][1], (shape, n, i))


# id -> (shape, kind, options that force it)
FRAMES = {
    "slide": ((333, 77, 4), SLIDE, ()),
    "pair": ((333, 77, 4), PAIR, ("NICE_ENC_NO_SLIDE",)),
    "ring": ((333, 77, 4), RING, ("NICE_ENC_NO_PAIR",)),
    "ring-rgb": ((333, 77, 3), RING, ()),
    "ring2": ((5000, 5, 4), RING2, ()),
    "ring2-rgb": ((5000, 5, 3), RING2, ()),
    "strip": ((5120, 6, 4), STRIP, ()),   # strips of 2048, 2048 and 1024 columns: two tiles per strip row, and one
    "twin": ((10300, 5, 4), TWIN, ()),
    "twin-rgb": ((10300, 5, 3), TWIN, ()),
    "window": ((333, 77, 4), WINDOW, ("NICE_ENC_NO_RING",)),
}
# batches whose blocks' tile ranges cross frame boundaries (the flush on a
# frame change): 26 and 15 tiles per frame against 16 per block; 11 x 51 = 561
# tiles > 2 x 256 blocks, two tiles per block on a 256-CU device
BATCHES = {
    "slide": ((333, 77, 4), 6, SLIDE, ()),
    "pair": ((333, 77, 4), 6, PAIR, ("NICE_ENC_NO_SLIDE",)),
    "ring": ((333, 77, 4), 6, RING, ("NICE_ENC_NO_PAIR",)),
    "ring-rgb": ((333, 77, 3), 6, RING, ()),
    "ring2": ((5000, 3, 4), 3, RING2, ()),
    "ring2-rgb": ((5000, 3, 3), 3, RING2, ()),
    "twin": ((10300, 5, 4), 11, TWIN, ()),
    "twin-rgb": ((10300, 5, 3), 11, TWIN, ()),
}
# R = 2 bands (no coded flags out: run digits counted inside the kernel)
BANDS = {
    "pair": ((333, 77, 4), PAIR),
    "ring-rgb": ((333, 77, 3), RING),
    "ring2": ((5000, 8, 4), RING2),
    "strip": ((5120, 8, 4), STRIP),
    "twin": ((10300, 6, 4), TWIN),
    "twin-rgb": ((10300, 6, 3), TWIN),
}


@pytest.mark.parametrize("case", FRAMES)
def test_stages_frame(nice, opts, case):
    shape, kind, options = FRAMES[case]
    _check_frames(nice, opts, shape, 1, kind, options)


@pytest.mark.parametrize("case", BATCHES)
def test_stages_batch(nice, opts, case):
    shape, n, kind, options = BATCHES[case]
    _check_frames(nice, opts, shape, n, kind, options)


@pytest.mark.parametrize("case", BANDS)
def test_stages_bands(nice, case):
    import torch
    from conftest import PKG_NAME
    S = importlib.import_module(PKG_NAME + ".sharded")
    (w, h, c), kind = BANDS[case]
    R = 2
    px, want = _run_input(w, h, c, 60)
    t = torch.from_numpy(px).cuda()
    backends = []
    got = S.encode_bands(t, w, h, c, R, backends=backends).cpu().numpy().tobytes()
    assert [_last(nice, be.ctx) for be in backends] == [kind] * R
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert [plan_driver.enc_plan(w, h, c, 1, cus, band=S.band_tiles(w, h, r, R))["kind_id"]
            for r in range(R)] == [kind] * R
    _same(got, want, (w, h, c))
