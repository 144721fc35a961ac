"""Every reference offset at every edge, through every classify kernel and
every row kernel.

The inputs are the planted-reference frames of tests/planted_refs.py: random
colours in which chosen pixels are made to take each back reference 1..4 and
each luma reference 0..10 at the row's first and last columns, at tile,
segment, wave, strip, block and band edges, and at the first pixel at which
the offset is valid.  tests/test_planted_refs_cpu.py proves from the oracle's
trace, with no GPU, that every such cell of every shape here is hit; each
shape has three frames (variants), which together hold every cell.

Encoder: the stream equals the oracle's bytes, the library reports the kernel
named here, and the planner names the same one (the slide kernels: one per
W mod 4).  Decoder: the oracle's stream of the frame decodes with status 0 to
the frame's pixels (alpha filled with 255 on four-channel output), by the
route named here, which is also the plan's."""
import importlib

import numpy as np
import pytest

import plan_driver
import planted_refs as P
from test_classify_routes import PAIR, RING, RING2, SLIDE, STRIP, TWIN, WINDOW, _last, _same
from test_classify_stages import _encode, _options

pytestmark = pytest.mark.gpu

# id -> (shape, kind, the options of test_classify_stages.FRAMES that force it)
ENC_CASES = {
    "slide0": ((332, 150, 4), SLIDE, ()),
    "slide1": ((333, 150, 4), SLIDE, ()),
    "slide2": ((334, 150, 4), SLIDE, ()),
    "slide3": ((335, 150, 4), SLIDE, ()),
    "pair": ((333, 150, 4), PAIR, ("NICE_ENC_NO_SLIDE",)),
    "ring": ((333, 150, 4), RING, ("NICE_ENC_NO_PAIR",)),
    "ring-rgb": ((333, 150, 3), RING, ()),
    "window": ((333, 150, 4), WINDOW, ("NICE_ENC_NO_RING",)),
    "ring2": ((5000, 24, 4), RING2, ()),
    "ring2-rgb": ((5000, 24, 3), RING2, ()),
    "strip": ((5120, 32, 4), STRIP, ()),   # class e; row 16 starts a block
    "twin": ((10300, 24, 4), TWIN, ()),
    "twin-rgb": ((10300, 24, 3), TWIN, ()),
}
_ROWS = {"NICE_DEC_FLOW": 0, "NICE_DEC_SPLIT": 0}
# id -> (kernel, the options of test_rows_store.ROUTES that force it, channels, shape)
DEC_CASES = {
    "rec-37": ("dec_reconstruct", {}, (3,), (37, 64, 3)),
    "rec-61": ("dec_reconstruct", {}, (3,), (61, 64, 3)),
    "rec1-67": ("dec_reconstruct", {"NICE_DEC_SINGLE_WAVE": 1}, (3,), (67, 64, 3)),
    "rows-67": ("dec_rows", _ROWS, (3,), (67, 64, 3)),       # the last segment: 3 pixels
    "rows-1026": ("dec_rows", _ROWS, (3, 4), (1026, 64, 3)),   # two waves; the last segment: 2 pixels
    "rows8-515": ("dec_rows8", {"NICE_DEC_SEG": 8}, (3,), (515, 64, 3)),
    "flow1-1026": ("dec_rows_flow", {"NICE_DEC_FLOW": 1}, (3, 4), (1026, 64, 3)),
    "flow2-1026": ("dec_rows_flow", {"NICE_DEC_FLOW": 2}, (3, 4), (1026, 64, 3)),
    "flow4-1026": ("dec_rows_flow", {"NICE_DEC_FLOW": 4}, (3, 4), (1026, 64, 3)),
    "flow2-67": ("dec_rows_flow", {"NICE_DEC_FLOW": 2}, (3,), (67, 64, 3)),
    "split2-1026": ("dec_rows_split", {"NICE_DEC_SPLIT": 2}, (3, 4), (1026, 64, 3)),
    "split3-1026": ("dec_rows_split", {"NICE_DEC_SPLIT": 3}, (3, 4), (1026, 64, 3)),
    "split2-67": ("dec_rows_split", {"NICE_DEC_SPLIT": 2}, (3,), (67, 64, 3)),   # strips of 3 and 2 segments
    # the ring in global memory (64-bit addresses), nine waves of which the last holds one segment
    "wide-8194": ("dec_rows_wide", {"NICE_DEC_SPLIT": 0}, (3,), (8194, 40, 3)),
    "split-8194": ("dec_rows_split", {}, (3,), (8194, 40, 3)),   # the default: three strips
}


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("case", ENC_CASES)
def test_encode_planted(nice, opts, case):
    shape, kind, options = ENC_CASES[case]
    w, h, c = shape
    plan_opts = _options(opts, options)
    ctx = nice.Context(0)
    for v in P.VARIANTS:
        px, want, _, _ = P.frame(shape, v)
        got, (al4, al16) = _encode(nice, [np.array(px)], w, h, c, ctx)
        assert _last(nice, ctx) == kind
        plan = plan_driver.enc_plan(w, h, c, 1, _cus(), al4=al4, al16=al16, **plan_opts)
        assert plan["kind_id"] == kind
        if kind == SLIDE:
            assert plan["kernel"] == f"enc_classify_slide{w % 4}"
        _same(got[0], want, (case, v))


@pytest.mark.parametrize("c", [3, 4])
def test_encode_planted_tiny(nice, c):
    """W = 1..7, where offsets coincide or wrap: whatever kernel the planner gives."""
    for w in range(1, 8):
        shape = (w, 40, c)
        assert shape in P.TINY_SHAPES
        ctx = nice.Context(0)
        for v in P.VARIANTS:
            px, want, _, _ = P.frame(shape, v)
            got, (al4, al16) = _encode(nice, [np.array(px)], w, 40, c, ctx)
            assert _last(nice, ctx) == plan_driver.enc_plan(w, 40, c, 1, _cus(), al4=al4, al16=al16)["kind_id"]
            _same(got[0], want, (shape, v))


@pytest.mark.parametrize("c,kind", [(4, PAIR), (3, RING)], ids=["pair", "ring-rgb"])
def test_encode_planted_bands(nice, c, kind):
    """Three bands: class d is planted at the band starts."""
    import torch
    from conftest import PKG_NAME
    S = importlib.import_module(PKG_NAME + ".sharded")
    w, h, R = 333, 150, 3
    assert [S.band_tiles(w, h, r, R)[0] * P.TILE for r in range(1, R)] == P.band_starts(w, h, R)
    for v in P.VARIANTS:
        px, want, _, cells = P.frame((w, h, c), v)
        assert {B for _, cls, B in cells if cls == "d"} >= set(P.band_starts(w, h, R))
        backends = []
        got = S.encode_bands(torch.from_numpy(np.array(px)).cuda(), w, h, c, R, backends=backends).cpu().numpy().tobytes()
        assert [_last(nice, be.ctx) for be in backends] == [kind] * R
        assert [plan_driver.enc_plan(w, h, c, 1, _cus(), band=S.band_tiles(w, h, r, R))["kind_id"]
                for r in range(R)] == [kind] * R
        _same(got, want, (c, v))


def test_encode_planted_batch(nice):
    """Two planted frames in one batch (blocks cross the frame boundary)."""
    shape = w, h, c = (333, 150, 4)
    frames = [P.frame(shape, v) for v in (0, 1)]
    ctx = nice.Context(0)
    got, (al4, al16) = _encode(nice, [np.array(f[0]) for f in frames], w, h, c, ctx)
    kind = plan_driver.enc_plan(w, h, c, 2, _cus(), al4=al4, al16=al16)["kind_id"]
    assert kind == SLIDE and _last(nice, ctx) == kind
    for i in range(2):
        _same(got[i], frames[i][1], i)


@pytest.mark.parametrize("case", DEC_CASES)
def test_decode_planted(nice, opts, case):
    import torch
    kernel, options, channels, (W, H, _) = DEC_CASES[case]
    for name, value in options.items():
        opts.setenv(name, value)
    want = plan_driver.plan(W, H, 1, _cus(), **{k[len("NICE_DEC_"):].lower(): v for k, v in options.items()})
    assert want["route"] == kernel
    # the properties the shapes were chosen for
    if W in (67, 1026) and kernel == "dec_rows":
        assert W % 16 == (3 if W == 67 else 2) and want["threads"] == (64 if W == 67 else 128)
    if case == "wide-8194":
        assert want["threads"] == 576 and W % 16 == 2
    if case == "split-8194":
        assert want["strips"] == 3 and P.strip_edges(W, 3) == [2736, 5472] and want["fallback"] == "dec_rows_wide"
    if case == "split2-67":
        assert (want["strips"], P.strip_edges(W, 2)) == (2, [48]) and (W + 15) // 16 == 5
    ctx = nice.Context(0)
    for C in channels:
        assert (W, H, C) in P.DEC_SHAPES
        for v in P.VARIANTS:
            px, s, _, _ = P.frame((W, H, C), v)
            rgb = px.reshape(-1, C)[:, :3]
            sb = torch.zeros((1, (len(s) + 255) // 256 * 256), dtype=torch.uint8)
            sb[0, :len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
            sb = sb.cuda()
            lens = torch.tensor([len(s)], dtype=torch.int64, device="cuda")
            for OC in (3, 4):
                dec = torch.zeros((1, W * H * OC), dtype=torch.uint8, device="cuda")
                status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
                nice.decode_batch(sb, lens, W, H, OC, dec, status,
                                  flags=nice.DEC_ALPHA_FILL_FF | nice.DEC_TOLERANT_HEADER, ctx=ctx)
                torch.cuda.synchronize()
                assert int(status[0]) == 0, (C, v, OC)
                assert plan_driver.last_route(nice, ctx) == (kernel, want["fallback"]), (C, v, OC)
                got = dec[0].view(-1, OC).cpu().numpy()
                if not np.array_equal(got[:, :3], rgb):
                    p = int(np.nonzero((got[:, :3] != rgb).any(axis=1))[0][0])
                    pytest.fail(f"C {C} variant {v} OC {OC}: first differing pixel {p} (row {p // W}, column {p % W}), "
                                f"trace byte {int(P.frame((W, H, C), v)[2][p]):#x}")
                if OC == 4:
                    assert (got[:, 3] == 255).all(), (C, v)
