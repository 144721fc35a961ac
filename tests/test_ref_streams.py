"""What no encoder emits, through every row kernel: hand-built streams
(tests/crafted_streams.py) in which every pixel draws its mode and its
reference uniformly among the valid ones.  So back reference 0 occurs (an
encoder writes a run instead), also at column 0, where it is the previous
row's last pixel; references that a lower index would match as well occur;
random payloads wrap in every mode; and chains of dependencies through
offsets 1, 2 and 3 run across segment, wave and strip edges, which is the row
kernels' speculative and fix-up path.

The shapes and routes are the decoder's of tests/test_ref_offsets.py, three
channels, 16 rows, every table at most 24 bits (so the reference's reader
finishes).  A test without a GPU asserts from what make_stream says it wrote
that back reference 0 and every luma reference occur at the row's first and
last columns (class a of tests/planted_refs.py), at a segment's first and
last columns (class f) and, where the shape has wave or strip edges, in the
six columns around each of them (class g: every edge on its own).  Pooling
is deliberate: a uniform draw gives a pixel one luma index in 50, so 16 rows
cannot fill single columns; the counts are pooled over each shape's streams
and over the columns of class a, of class f and of each edge, and back
reference 0 is pinned at column 0 itself.  The
reference is the oracle's literal decode; the GPU must equal it in the
default mode and with DEC_STRICT_REFERENCE."""
import functools

import numpy as np
import pytest

import crafted_streams as C
import plan_driver
import planted_refs as P
from test_ref_offsets import DEC_CASES

H = 16
WIDTHS = sorted({shape[0] for _, _, _, shape in DEC_CASES.values()})
# streams per width (seeds at which the pooled classes below hold every reference)
SEEDS = {37: (1, 2, 3), 61: (1, 2, 3), 67: (1, 2, 3), 515: (1, 2, 7), 1026: (1, 2, 3), 8194: (1, 2, 6)}
KINDS = [(0, 0)] + [(2, k) for k in range(11)]


@functools.lru_cache(maxsize=None)
def _streams(W):
    """[(stream, what each pixel was written as, the oracle's reference decode)] of a width."""
    from conftest import oracle_mod
    O = oracle_mod()
    out = []
    for seed in SEEDS[W]:
        s, info = C.make_stream(O, 1000 * W + seed, W=W, H=H, deep=C.NO_DEEP, uniform=True, run_p=0.05, run_max=8)
        assert info["max"] <= 24
        ref, dims = O.decode(s)
        assert dims == (W, H, 3)
        out.append((s, info["pixels"], ref))
    return out


@pytest.mark.parametrize("W", WIDTHS)
def test_streams_hold_every_reference_at_the_edges(W):
    edges = sorted({e for (w, _, _), es in P.DEC_SHAPES.items() if w == W for e in es})
    classes = {"a": {0, 1, 2, 3, W - 4, W - 3, W - 2, W - 1},
               "f": {x for x in range(W) if x % 16 in (0, 1, 2, 13, 14, 15)},
               **{f"g{e}": set(range(e - 3, min(e + 3, W))) for e in edges}}
    seen = {cls: set() for cls in classes}
    col0 = 0
    for _, pixels, _ in _streams(W):
        for p, what in enumerate(pixels):
            if what is not None:
                for cls, cols in classes.items():
                    if p % W in cols:
                        seen[cls].add(what)
                col0 += what == (0, 0) and p % W == 0
    for cls, cols in classes.items():
        assert cols and set(KINDS) <= seen[cls], (cls, sorted(set(KINDS) - seen[cls]))
    assert bool(edges) == (W >= 67)
    assert col0 >= 1
    # every mode, every back reference too, and runs
    assert {m for cls in seen.values() for m, _ in cls} == set(range(5))
    assert {k for m, k in seen["f"] if m == 0} == set(range(5))
    assert any(what is None for _, pixels, _ in _streams(W) for what in pixels)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEC_CASES)
def test_crafted_streams_decode(nice, opts, case):
    import torch
    kernel, options, _, (W, _, _) = DEC_CASES[case]
    for name, value in options.items():
        opts.setenv(name, value)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    want = plan_driver.plan(W, H, 1, cus, **{k[len("NICE_DEC_"):].lower(): v for k, v in options.items()})
    assert want["route"] == kernel
    if W == 8194:
        assert (want["threads"] == 576) if kernel == "dec_rows_wide" else (want["strips"] == 3)
    ctx = nice.Context(0)
    for i, (s, _, ref) in enumerate(_streams(W)):
        sb = torch.zeros((1, (len(s) + 255) // 256 * 256), dtype=torch.uint8)
        sb[0, :len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
        sb = sb.cuda()
        lens = torch.tensor([len(s)], dtype=torch.int64, device="cuda")
        for flags in (0, nice.DEC_STRICT_REFERENCE):
            dec = torch.zeros((1, W * H * 3), dtype=torch.uint8, device="cuda")
            status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            nice.decode_batch(sb, lens, W, H, 3, dec, status, flags=flags, ctx=ctx)
            torch.cuda.synchronize()
            assert int(status[0]) == 0, (i, flags)
            assert plan_driver.last_route(nice, ctx) == (kernel, want["fallback"]), (i, flags)
            got = dec[0].cpu().numpy()
            if not np.array_equal(got, ref):
                p = int(np.nonzero(got != ref)[0][0]) // 3
                pytest.fail(f"stream {i} flags {flags}: first differing pixel {p} (row {p // W}, column {p % W}), "
                            f"written as {_streams(W)[i][1][p]}")
