"""The event word dec_sync keeps per parsed pixel, laid out like the record, and
dec_place's record from it (csrc/nice_dec_event.hpp: ev_pack, place_record).

Every decode here runs twice: with the default routes (the parse keeps its
events, dec_place turns them into records) and with NICE_DEC_NO_EVENTS, which
sends every slice through dec_emit and make_record, the yardstick.  Pixels and
the frame's status must be identical.  The inputs: SYN-v1 frames, planted
reference frames (tests/planted_refs.py: every reference at the row's first and
last columns and around segment edges) at the same small widths, hand-built
streams that take the fast parse, and crafted streams the reference rejects --
a reference before the image start, LUMA2 on the first row, and a back
reference id past the five that exist, deep in the image, where dec_place's
steps run without position checks.  Each is repeated with 1024- and 16384-bit
slices (the 256-event steps of dec_place then start on both sides of pixel
3W + 3, the hoisting rule's line), on the general parse, and with a head buffer
every head overflows.

tests/test_dec_event_arith.py checks the same arithmetic exhaustively on the
CPU."""
import functools

import numpy as np
import pytest

import crafted_streams as C
import parse_streams as PS
import planted_refs as P

SHAPES = [(67, 40, 3), (130, 33, 4), (512, 96, 4)]
MODES = ["default", "slice1024", "slice16384", "slow_parse", "small_hev"]
BAD_KINDS = ["ref_before_start", "luma2_first_row", "rejected_id_deep"]


def _set_mode(opts, mode):
    opts.reset()
    if mode == "slice1024":
        opts.setenv("NICE_DEC_SLICE_BITS", 1024)
    if mode == "slice16384":
        opts.setenv("NICE_DEC_SLICE_BITS", 16384)
    if mode == "slow_parse":
        opts.setenv("NICE_DEC_SLOW_PARSE", 1)
    if mode == "small_hev":   # 4 events: no head fits (a head is at least 512 bits, an event at most 64)
        opts.setenv("NICE_DEC_SLICE_BITS", 1024)
        assert opts.L.nice_test_set_option(PS.OPT_DEC_HEV_CAP, 4) == 0


def _decode(nice, s, W, H, c, flags):
    """(pixels, status) of one stream through decode_batch."""
    import torch
    sb = torch.zeros((1, (len(s) + 255) // 256 * 256), dtype=torch.uint8)
    sb[0, :len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
    sb = sb.cuda()
    lens = torch.tensor([len(s)], dtype=torch.int64, device="cuda")
    dec = torch.zeros((1, W * H * c), dtype=torch.uint8, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    nice.decode_batch(sb, lens, W, H, c, dec, status, flags=flags)
    torch.cuda.synchronize()
    return dec[0].cpu().numpy(), int(status[0])


def _both(nice, opts, mode, s, W, H, c, encoded=False):
    """The decode on the default routes and through dec_emit alone.  encoded:
    the stream comes from the encoder; frames this small have table headers
    only DEC_TOLERANT_HEADER reads (tests/test_tolerant.py)."""
    flags = nice.DEC_ALPHA_FILL_FF | nice.DEC_TOLERANT_HEADER if encoded else 0
    _set_mode(opts, mode)
    ev = _decode(nice, s, W, H, c, flags)
    opts.setenv("NICE_DEC_NO_EVENTS", 1)
    no_ev = _decode(nice, s, W, H, c, flags)
    return ev, no_ev


@functools.lru_cache(maxsize=None)
def _syn(shape):
    from conftest import oracle_mod
    O = oracle_mod()
    w, h, c = shape
    px = O.gen_syn_v1(w, h, c, 3)
    return O.encode(px, w, h, c), px.reshape(-1, c)[:, :3].copy()


@functools.lru_cache(maxsize=None)
def _planted(shape, variant):
    """A planted-reference frame of the shape (not one of planted_refs' own
    shapes: its table, without block starts, at a seed of this file) and what
    the oracle's trace says its pixels took."""
    from conftest import oracle_mod
    O = oracle_mod()
    w, h, c = shape
    cells = P.cell_table(w, h, variant, decoder=True, edges=P.wave_edges(w, 8))
    px = P.planted_frame(w, h, c, 900 + 10 * w + variant, cells)
    s, trace = O.encode_trace(px, w, h, c)
    return s, px.reshape(-1, c)[:, :3].copy(), np.asarray(trace)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_planted_frames_hold_every_reference(shape):
    """Over a shape's three frames every back and luma reference is taken, at
    the row's first and last columns too."""
    w = shape[0]
    seen, edge = set(), set()
    for variant in P.VARIANTS:
        trace = _planted(shape, variant)[2]
        for kind in P.KINDS:
            pos = np.nonzero(trace == P.CODE(kind))[0]
            if pos.size:
                seen.add(kind)
            if np.isin(pos % w, [0, 1, 2, 3, w - 4, w - 3, w - 2, w - 1]).any():
                edge.add(kind)
    assert seen == set(P.KINDS) and edge == set(P.KINDS), (sorted(set(P.KINDS) - seen), sorted(set(P.KINDS) - edge))


def _lens_flat(O, rng):
    return C._profile_lengths(O, rng, "flat")


@functools.lru_cache(maxsize=None)
def _bad_stream(kind, W=67, H=40):
    """A grammar-valid stream on the "flat" tables (the fast parse) with one
    pixel the reference rejects; every other pixel draws a valid mode and
    reference.  Returns (stream, the bad pixel's index)."""
    from conftest import oracle_mod
    O = oracle_mod()
    rng = np.random.default_rng(77)
    N = W * H
    lens = _lens_flat(O, rng)
    codes = [O.canonical(l) for l in lens]
    b = C._Bits()
    for st in range(10):
        b.put(int(lens[st].max()), 5)
        for v in lens[st]:
            b.put(int(v), 7)

    def sym(st, v):
        b.put(int(codes[st][v]), int(lens[st][v]))

    at = {"ref_before_start": W + 1, "luma2_first_row": 3, "rejected_id_deep": 20 * W + 9}[kind]
    i = 0
    while i < N:
        if i == at and kind == "ref_before_start":
            sym(1, 2); sym(4, 6); sym(2, 40); sym(3, 20); sym(3, 9)       # LUMA, 3W back
        elif i == at and kind == "luma2_first_row":
            sym(1, 4); sym(6, 33); sym(7, 17); sym(8, 2)
        elif i == at:
            sym(1, 0); sym(9, 7)                                          # BACK_REF has ids 0..4
        else:
            mode = 1 if i == 0 else int(rng.integers(5 if i >= W else 4))
            if mode == 0:
                sym(1, 0); sym(9, int(rng.choice([k for k, o in enumerate(C.BR_OFF(W)) if 0 < o <= i])))
            elif mode == 1:
                sym(1, 1); sym(0, rng.integers(256)); sym(0, rng.integers(256)); sym(0, rng.integers(256))
            elif mode == 2:
                sym(1, 2); sym(4, int(rng.choice([k for k, o in enumerate(C.LUMA_OFF(W)) if 0 < o <= i])))
                sym(2, rng.integers(64)); sym(3, rng.integers(32)); sym(3, rng.integers(32))
            elif mode == 3:
                sym(1, 3); sym(5, rng.integers(343))
            else:
                sym(1, 4); sym(6, rng.integers(64)); sym(7, rng.integers(32)); sym(8, rng.integers(32))
        i += 1
        if i != at and i < N - 12 and rng.random() < 0.1:
            r = int(rng.integers(1, 10))
            if i < at <= i + r:
                continue
            m = r - 1
            while True:
                sym(1, 5 + m % 8)
                if m < 8:
                    break
                m //= 8
            i += r
    sym(1, 1)
    hdr = b"nice" + W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([3])
    return hdr + b.tobytes() + bytes(8), at


@pytest.mark.parametrize("kind", BAD_KINDS)
def test_bad_streams_are_rejected_by_the_oracle(O, kind):
    s, at = _bad_stream(kind)
    assert C.lut_plan(PS.maxes(s))[3], "the fast parse"
    assert (at >= 3 * 67 + 3) == (kind == "rejected_id_deep")
    for mode in (O.DEC_REFERENCE, O.DEC_STRIDE):
        with pytest.raises(O.OracleDecodeError):
            O.decode(s, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_syn_frames(nice, opts, shape, mode):
    w, h, c = shape
    s, want = _syn(shape)
    (got, st), (got0, st0) = _both(nice, opts, mode, s, w, h, c, encoded=True)
    assert st == st0 == 0
    assert np.array_equal(got, got0)
    assert np.array_equal(got.reshape(-1, c)[:, :3], want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_planted_frames(nice, opts, shape, mode):
    w, h, c = shape
    for variant in P.VARIANTS:
        s, want, _ = _planted(shape, variant)
        (got, st), (got0, st0) = _both(nice, opts, mode, s, w, h, c, encoded=True)
        assert st == st0 == 0, variant
        assert np.array_equal(got, got0), variant
        assert np.array_equal(got.reshape(-1, c)[:, :3], want), variant


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width", [PS.W_SMALL, PS.W_MAIN])
def test_fast_parse_streams(nice, opts, width, mode):
    """Hand-built streams on tables the fast parse takes (the event word then
    comes from the shifts in the parameter words): every mode and reference
    drawn uniformly."""
    W, seed = [(w, sd) for w, sd in PS.STREAMS["flat"] if w == width][0]
    s, _, ref, _ = PS.stream("flat", W, seed)
    (got, st), (got0, st0) = _both(nice, opts, mode, s, W, PS.H, 3)
    assert st == st0 == 0
    assert np.array_equal(got, got0)
    assert np.array_equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", BAD_KINDS)
def test_rejected_streams(nice, opts, kind, mode):
    s, _ = _bad_stream(kind)
    (_, st), (_, st0) = _both(nice, opts, mode, s, 67, 40, 3)
    assert st == st0 == nice.E_FORMAT, (st, st0)
