"""The planted-reference frames (tests/planted_refs.py) on the CPU, before any
GPU comparison: the oracle's trace is consistent with its stream, every cell
of every shape's table is hit in the trace, the first valid pixel of every
reference takes it and the pixel before does not, and every decoder shape
round-trips through the oracle's tolerant decode.  No cell is dropped and no
shape skipped: tests/test_ref_offsets.py feeds exactly these frames to the
kernels."""
import time

import numpy as np
import pytest

import planted_refs as P

SHAPES = list(P.ENC_SHAPES) + list(P.DEC_SHAPES)
ALL = SHAPES + P.TINY_SHAPES
_id = lambda s: "x".join(map(str, s))


def test_generator_is_deterministic_and_quick():
    shape = (8194, 40, 3)   # the largest table here: ten wave and strip edges
    cells = P.table(shape, 0)
    assert len(P.DEC_SHAPES[shape]) == 10 and len(cells) > 1500
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        a = P.planted_frame(*shape, 11, cells)
        times.append(time.perf_counter() - t0)
    # the work is bounded by the table, not the frame: Python touches the planted pixels only
    # (each cell at most REPEATS times, moved a few times when shadowed, plus the sprinkle)
    N = shape[0] * shape[1]
    assert P.planted_frame.plantings <= 2 * P.REPEATS * len(cells) + N // P.SPRINKLE < N // 20
    assert min(times) < 1.0, times   # about 0.2 s here; the best of three, so a busy machine does not fail it
    assert np.array_equal(a, P.planted_frame(*shape, 11, cells))
    assert not np.array_equal(a, P.planted_frame(*shape, 12, cells))


@pytest.mark.parametrize("shape", ALL, ids=_id)
def test_trace_matches_stream(O, shape):
    """encode_trace writes encode's bytes, and its trace adds up to encode's
    own counts: run members, pixels per mode, the two reference histograms."""
    W, H, C = shape
    for v in P.VARIANTS:
        px, stream, trace, _ = P.frame(shape, v)
        want, st = O.encode(px, W, H, C, with_stats=True)
        assert stream == want, v
        assert trace.shape == (W * H,)
        # (W = 1: back reference 2 has offset W - 1 = 0, and pixel 0 equals itself)
        assert trace[0] == (O.T_RGB << 4 if W > 1 else O.T_BACK << 4 | 2)
        run = trace == O.T_RUN
        mode = trace[~run] >> 4
        assert int(run.sum()) == st.n_run_pixels and int((~run).sum()) == st.n_coded
        assert [int((mode == m).sum()) for m in (O.T_BACK, O.T_RGB, O.T_LUMA, O.T_SMALL, O.T_LUMA2)] == \
            [st.n_backref, st.n_rgb, st.n_luma, st.n_smalldiff, st.n_luma2]
        assert not (trace[~run][(mode != O.T_BACK) & (mode != O.T_LUMA)] & 15).any()
        first = np.cumsum([0] + O.STREAM_N)   # the histogram's streams, in id order (4: luma, 9: back references)
        assert [int((trace == (O.T_LUMA << 4 | k)).sum()) for k in range(11)] == list(st.hist[first[4]:first[4] + 11])
        assert [int((trace == (O.T_BACK << 4 | k)).sum()) for k in range(5)] == list(st.hist[first[9]:first[9] + 5])
        assert st.hist[first[9]] == 0   # back reference 0 is never emitted: such a pixel is a run member


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_every_cell_is_hit(shape):
    """Every cell of each variant's table has a hit in the oracle's trace, and
    the three tables together hold every kind in every class."""
    W, H, C = shape
    union = set()
    for v in P.VARIANTS:
        _, _, trace, cells = P.frame(shape, v)
        assert len(set(cells)) == len(cells)
        hits = P.coverage(trace, W, cells)
        empty = [c for c in cells if hits[c] == 0]
        assert not empty, (v, empty)
        union |= set(cells)
    classes = {(cls, arg) for _, cls, arg in union if cls not in "c"}
    assert classes and union == {(k, cls, arg) for k in P.KINDS for cls, arg in classes} | \
        {(k, "c", P.offset(k, W)) for k in P.KINDS}
    assert {c[1] for c in union} >= set("ac" + ("bd" if W * H >= 24 * P.TILE else "") +
                                        ("e" if P.ENC_SHAPES.get(shape, {}).get("strip") else "") +
                                        ("f" if shape in P.DEC_SHAPES else "") +
                                        ("g" if P.DEC_SHAPES.get(shape) else ""))


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_first_valid_pixel(shape):
    """Pixel off_k references pixel 0 through k and takes it (in the variant
    that can hold it); pixel off_k - 1 never does."""
    W = shape[0]
    for kind in P.KINDS:
        off = P.offset(kind, W)
        took = [int(P.frame(shape, v)[2][off]) == P.CODE(kind) for v in P.VARIANTS]
        assert all(t for t, v in zip(took, P.VARIANTS) if kind not in P.C_LEFT_OUT[v]), (kind, took)
        assert any(kind not in P.C_LEFT_OUT[v] for v in P.VARIANTS)
        assert all(int(P.frame(shape, v)[2][off - 1]) != P.CODE(kind) for v in P.VARIANTS), kind


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_luma_deltas_reach_the_window_edges(shape):
    """Among the pixels that took a luma reference: both ends of each delta
    range, and sums that wrap past 255 and below 0."""
    W, H, C = shape
    g, e, wrap = set(), set(), set()
    for v in P.VARIANTS:
        px, _, trace, _ = P.frame(shape, v)
        rgb = px.reshape(-1, C)[:, :3].astype(np.int64)
        for k in range(11):
            p = np.nonzero(trace == (2 << 4 | k))[0]
            ref = rgb[p - P.LUMA_OFF(W)[k]]
            dg = (rgb[p, 1] - ref[:, 1] + 32) % 256 - 32
            g |= set(dg.tolist())
            for c in (0, 2):
                e |= set(((rgb[p, c] - ref[:, c] - dg + 16) % 256 - 16).tolist())
            wrap |= set(np.sign(ref[:, 1] + dg - rgb[p, 1]).tolist())
    assert {-32, 31} <= g <= set(range(-32, 32)) and {-16, 15} <= e <= set(range(-16, 16))
    assert wrap == {-1, 0, 1}


@pytest.mark.parametrize("shape", list(P.DEC_SHAPES), ids=_id)
def test_decoder_shapes_round_trip(O, shape):
    """The oracle's tolerant decode returns every decoder frame (the header's
    channel byte set to 3, as the GPU tests decode it)."""
    W, H, C = shape
    for v in P.VARIANTS:
        px, s, _, _ = P.frame(shape, v)
        ref, dims = O.decode(s[:12] + bytes([3]) + s[13:], O.DEC_TOLERANT)
        assert dims == (W, H, 3)
        assert np.array_equal(ref.reshape(-1, 3), px.reshape(-1, C)[:, :3]), v


def test_tiny_shapes_hold_references():
    """W = 1..7: offsets coincide (W = 2: W-1 and 1) or are not positive (W-1,
    W-3); from W = 2 the frames still make the encoder take back and luma
    references."""
    for shape in P.TINY_SHAPES:
        codes = set()
        for v in P.VARIANTS:
            codes |= set(P.frame(shape, v)[2].tolist())
        if shape[0] == 1:   # back reference 2 (offset W - 1 = 0: the pixel itself) always matches
            assert codes <= {2, 0xFF}, sorted(codes)
        else:
            assert len({c for c in codes if c >> 4 == 2}) >= 3 and any(c >> 4 == 0 for c in codes), (shape, sorted(codes))
