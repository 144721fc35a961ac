"""Slice heads placed from the re-parses' kept events (dec_sync -> dec_place).

A re-parse of a slice (dec_sync with its entry corrected) keeps its pixel
events up to the checkpoint where it meets the previous parse; dec_place then
writes the slice's records from those events and, past the meeting point, from
the first pass's, so dec_emit has no head to parse again.  A head that cannot
be trusted (more events than the buffer holds, no meeting point, a later
re-parse that met earlier than the latest meeting point) keeps the older path:
dec_heads lists it and dec_emit parses it.

Every case compares pixels and status with the oracle's decode, at small
shapes cut into many slices (slice size forced to 1024 and 4096 bits).
"""
import numpy as np
import pytest

import crafted_streams as C
import parse_streams as PS
from parse_streams import OPT_DEC_HEV_CAP
DATA_START_BITS = 13 * 8 + 6056   # file header + the ten table headers

SHAPES = [(256, 256, 4), (256, 256, 3), (257, 130, 4), (257, 130, 3)]
SLICES = [1024, 4096]

_cache = {}


def _syn(O, w, h, c, seed=1):
    """(stream, the oracle's decode of it as RGB rows), computed once."""
    key = (w, h, c, seed)
    if key not in _cache:
        s = O.encode(O.gen_syn_v1(w, h, c, seed), w, h, c)
        want = O.decode(s, O.DEC_STRIDE)[0].reshape(-1, c)[:, :3].copy()
        want.setflags(write=False)
        _cache[key] = (s, want)
    return _cache[key]


def _n_slices(s, slice_bits):
    return -(-(len(s) * 8 - DATA_START_BITS) // slice_bits)


def _gpu_rgb(nice, s, c, flags=None):
    got = nice.decode_bytes(s) if flags is None else nice.decode_bytes(s, flags)
    return np.frombuffer(got[0], np.uint8).reshape(-1, c)[:, :3]


def _set_hev_cap(opts, v):
    assert opts.L.nice_test_set_option(OPT_DEC_HEV_CAP, v) == 0


_head_stats = PS.head_stats   # the 'slice heads' line of the decoder's statistics as a dict


def test_streams_have_many_slices(O):
    """The shapes give hundreds of slices, and one a count that is no multiple
    of 64 (the event groups of a frame are padded to 64 slices)."""
    s, _ = _syn(O, 256, 256, 4)
    assert _n_slices(s, 1024) >= 500
    counts = [_n_slices(_syn(O, w, h, c)[0], b) for (w, h, c) in SHAPES for b in SLICES]
    assert any(n % 64 for n in counts), counts


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["default", "slow_parse", "small_hev", "slow_parse_small_hev"])
@pytest.mark.parametrize("slice_bits", SLICES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_decode_matches_oracle(nice, O, opts, capfd, shape, slice_bits, mode):
    """With the heads placed (default) and with a head buffer of 4 events,
    which every head overflows, so dec_emit parses them as before: the same
    pixels either way.

    All four shapes take the general parse: their SMALL_DIFF table has 17 bits
    and their LUMA2_BASE table 13, over the 12-bit first level, so
    DecTables::fast is 0 and "default" runs the code "slow_parse" forces (the
    statistics' parse line is asserted to say so).  The fast parse at these
    slice sizes is tests/test_parse_paths.py's, on a 512x512 frame and on
    hand-built streams."""
    w, h, c = shape
    s, want = _syn(O, w, h, c)
    lut_bits, long_streams, _, fast = C.lut_plan(PS.maxes(s))
    assert long_streams == [5, 6] and not fast
    opts.setenv("NICE_DEC_SLICE_BITS", slice_bits)
    opts.setenv("NICE_DEC_STATS", 1)
    if "slow_parse" in mode:
        opts.setenv("NICE_DEC_SLOW_PARSE", 1)
    if "small_hev" in mode:
        _set_hev_cap(opts, 4)
    got = _gpu_rgb(nice, s, c)
    assert np.array_equal(got, want)
    err = capfd.readouterr().err
    ps = PS.parse_stats(err)
    assert (ps["frames"], ps["fast"], ps["max"], ps["lut_bits"]) == (1, 0, PS.maxes(s), lut_bits), ps
    assert ps["slow_parse"] == int("slow_parse" in mode), ps
    st = _head_stats(err)
    print(st)
    assert st["invariant_violations"] == 0
    assert sum(st[k] for k in ("none", "placed", "emitted", "whole_slice_emitted")) == _n_slices(s, slice_bits)
    if "small_hev" in mode:
        # an event is at most 64 bits, a head at least one checkpoint (512
        # bits) long: more than 4 events, so none fits
        assert st["placed"] == 0 and st["emitted"] > 0, st
    else:
        assert st["placed"] > 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("slice_bits", SLICES)
def test_heads_are_placed_not_emitted(nice, O, opts, capfd, slice_bits):
    """On plain SYN-v1 frames the re-parses meet the previous parse within the
    first two checkpoints (the oracle's parse shows it on the CPU), and the
    head buffer holds the events up to the second checkpoint.  So with slices
    that have two checkpoints or more (4096 bits: seven, 512 bits apart) at
    most 5 % of the slices may take a dec_emit fallback, head or whole slice.
    A 1024-bit slice has a single checkpoint, 512 bits in: a re-parse that has
    not met the previous parse there cannot meet it at all, and dec_emit
    parses the whole slice, as it did before the heads were kept (13 % of
    these slices when this test was written).  There the cap is on what this
    path decides: of the slices whose parses did meet, at most 5 % may have
    their head parsed by dec_emit.  No head may end anywhere but at its
    meeting point."""
    tot = {"none": 0, "placed": 0, "emitted": 0, "whole_slice_emitted": 0, "invariant_violations": 0}
    opts.setenv("NICE_DEC_SLICE_BITS", slice_bits)
    opts.setenv("NICE_DEC_STATS", 1)
    for (w, h, c) in SHAPES:
        s, want = _syn(O, w, h, c)
        assert np.array_equal(_gpu_rgb(nice, s, c), want)
        st = _head_stats(capfd.readouterr().err)
        for k in tot:
            tot[k] += st[k]
    n = tot["none"] + tot["placed"] + tot["emitted"] + tot["whole_slice_emitted"]
    fallback = tot["emitted"] + tot["whole_slice_emitted"]
    print(f"slice {slice_bits}: {tot}, fallback share {fallback / n:.4f}, "
          f"heads parsed by dec_emit {tot['emitted'] / n:.4f}")
    assert tot["invariant_violations"] == 0
    assert tot["placed"] > 0
    if slice_bits >= 2048:
        assert fallback <= 0.05 * n, tot
    else:
        assert tot["emitted"] <= 0.05 * (n - tot["whole_slice_emitted"]), tot


@pytest.mark.gpu
def test_slow_sync_stream_takes_the_fallback(nice, O, opts, capfd):
    """tests/crafted_streams.make_slow_sync: a wrong parse re-synchronises only
    after thousands of bits, so slices are re-parsed many times, most re-parses
    never meet the previous one inside their slice, and the device settle ends
    the iteration: heads whose kept events do not belong to the latest meeting
    point must go to dec_emit, and the pixels stay exact."""
    W, H = 256, 256
    s = C.make_slow_sync(O, 5, W, H)
    want = O.decode(s)[0]
    opts.setenv("NICE_DEC_SLICE_BITS", 1024)
    opts.setenv("NICE_DEC_STATS", 1)
    got = np.frombuffer(nice.decode_bytes(s)[0], np.uint8)
    assert np.array_equal(got, want)
    err = capfd.readouterr().err
    st = _head_stats(err)
    line = [l for l in err.splitlines() if "sync iterations that changed an entry" in l][-1]
    flags = [int(x) for x in line.split(":")[1].split("(")[0].split()]
    print(st, flags)
    assert flags[16] == 1 and flags[17] == 0, line   # settled on the device; the final iteration moved nothing
    assert st["invariant_violations"] == 0
    assert st["emitted"] + st["whole_slice_emitted"] > 0, st
    opts.setenv("NICE_DEC_SLICE_BITS", 4096)
    got = np.frombuffer(nice.decode_bytes(s)[0], np.uint8)
    assert np.array_equal(got, want)
    assert _head_stats(capfd.readouterr().err)["invariant_violations"] == 0


@pytest.mark.gpu
def test_pipeline_one_queued_iteration(nice, O, opts):
    """The pipeline's decode with one queued sync iteration: the settle and the
    iteration behind it re-parse most slices, and their heads are placed."""
    opts.setenv("NICE_DEC_SYNC_QUEUED", 1)
    opts.setenv("NICE_DEC_SLICE_BITS", 1024)
    w, h, c, n = 160, 96, 4, 5
    frames = [O.gen_syn_v1(w, h, c, 40 + i) for i in range(n)]
    p = nice.Pipeline(w, h, c, batch=2, depth=2)
    outs = [np.zeros(p.stream_stride, np.uint8) for _ in range(n)]
    lens = p.encode(frames, outs)
    dec = [np.zeros(w * h * c, np.uint8) for _ in range(n)]
    assert p.decode(outs, lens, dec) == [0] * n
    for i in range(n):
        want = O.decode(outs[i][:lens[i]].tobytes(), O.DEC_STRIDE)[0].reshape(-1, c)[:, :3]
        assert np.array_equal(dec[i].reshape(-1, c)[:, :3], want), i
    p.close()


def _mixed_batch(O):
    """Six 256x256 RGBA streams of clearly different lengths: SYN-v1 frames,
    one of them with noise in its low bits (a longer stream), one a 128x128
    frame with every pixel doubled (a much shorter one)."""
    w, h, c = 256, 256, 4
    rng = np.random.default_rng(9)
    frames = []
    for i in range(6):
        px = O.gen_syn_v1(w, h, c, 11 + i).copy()
        if i == 1:
            px ^= rng.integers(0, 16, px.size, dtype=np.uint8)
        if i == 4:
            small = O.gen_syn_v1(w // 2, h // 2, c, 11 + i).reshape(h // 2, w // 2, c)
            px = np.repeat(np.repeat(small, 2, 0), 2, 1).reshape(-1).copy()
        frames.append(px)
    streams = [O.encode(f, w, h, c) for f in frames]
    wants = [O.decode(s, O.DEC_STRIDE)[0].reshape(-1, c)[:, :3] for s in streams]
    return w, h, c, streams, wants


def test_mixed_batch_lengths_differ(O):
    _, _, _, streams, _ = _mixed_batch(O)
    ls = sorted(len(s) for s in streams)
    assert ls[0] * 1.3 < ls[-1], ls


@pytest.mark.gpu
@pytest.mark.parametrize("slice_bits", SLICES)
def test_batch_with_corrupt_header(nice, O, opts, slice_bits):
    """Frames of different stream lengths in one batch, the header of one in
    the middle corrupt: that frame fails, the others decode exactly."""
    import torch
    opts.setenv("NICE_DEC_SLICE_BITS", slice_bits)
    w, h, c, streams, wants = _mixed_batch(O)
    n = len(streams)
    stride = (max(len(s) for s in streams) + 255) // 256 * 256
    buf = np.zeros((n, stride), np.uint8)
    for i, s in enumerate(streams):
        buf[i, :len(s)] = np.frombuffer(s, np.uint8)
    buf[3, 4:8] = [0, 0, 0, 9]   # another width than the batch's
    st_dev = torch.from_numpy(buf).cuda()
    lens = torch.tensor([len(s) for s in streams], dtype=torch.int64, device="cuda")
    dec = torch.zeros((n, w * h * 4), dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    nice.decode_batch(st_dev, lens, w, h, 4, dec, status)
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    assert st[3] == nice.E_ARG and [st[i] for i in (0, 1, 2, 4, 5)] == [0] * 5, st
    got = dec.cpu().numpy().reshape(n, -1, 4)[:, :, :3]
    for i in (0, 1, 2, 4, 5):
        assert np.array_equal(got[i], wants[i]), i


# ---- streams that end in a way only the decoder's end rules decide ---------
END_KINDS = ["digit_at_n", "zero_digits_at_n", "run_past_n"]
END_SEEDS = range(6)


def _crafted_end(O, seed, kind, W=96, H=48):
    """A random grammar-valid stream (as crafted_streams.make_stream, every
    table at most 24 bits) with a chosen end:
      digit_at_n        the extra prefix after the last pixel is a run digit
                        (strict: the reference copies past its buffer)
      zero_digits_at_n  a run ends exactly at the last pixel, zero digits of it
                        follow, then the extra prefix is a coded pixel's
      run_past_n        the last run is longer than the pixels left
    Returns (stream, end_in_head): whether the end lies in the first 512 bits
    of its 1024-bit slice, where a re-parse's head would hold it."""
    key = ("end", seed, kind, W, H)
    if key not in _cache:
        _cache[key] = _build_crafted_end(O, seed, kind, W, H)
    return _cache[key]


def _build_crafted_end(O, seed, kind, W, H):
    rng = np.random.default_rng(1000 + seed)
    N = W * H
    lens = [C._lengths(O, rng, n) for n in C.SIZES]
    codes = [O.canonical(l) for l in lens]
    b = C._Bits()
    for st in range(10):
        b.put(int(lens[st].max()), 5)
        for v in lens[st]:
            b.put(int(v), 7)

    def sym(st, v):
        b.put(int(codes[st][v]), int(lens[st][v]))

    def run(r):
        m = r - 1
        while True:
            sym(1, 5 + m % 8)
            if m < 8:
                break
            m //= 8

    tail_run = int(rng.integers(3, 30))   # pixels the last run covers (or would have to)
    i = 0
    while i < N:
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
        if kind != "digit_at_n" and i == N - tail_run:
            break
        if i < N - 40 and rng.random() < 0.25:
            r = int(rng.integers(1, 40))
            run(r)
            i += r
    end_bit = len(b.bits) - 6056
    if kind == "digit_at_n":
        sym(1, 5 + int(rng.integers(1, 8)))
    elif kind == "zero_digits_at_n":
        run(tail_run)
        sym(1, 5); sym(1, 5)
        sym(1, int(rng.integers(5)))
    else:
        run(tail_run + int(rng.integers(1, 200)))
    hdr = b"nice" + W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([3])
    return hdr + b.tobytes() + bytes(rng.integers(0, 256, 3, dtype=np.uint8)) + bytes(5), end_bit % 1024 < 512


def _oracle_outcome(O, s, mode):
    try:
        return O.decode(s, mode)[0]
    except O.OracleDecodeError as e:
        return e


def test_crafted_ends_cover_heads_and_outcomes(O):
    """Each kind of end falls into a slice's head for some seed and past it
    for another, and the oracle decides them as the format says: a run past
    the last pixel fails in both modes, a run digit as the extra prefix only
    in the reference's."""
    for kind in END_KINDS:
        in_head = set()
        for seed in END_SEEDS:
            s, head = _crafted_end(O, seed, kind)
            in_head.add(head)
            ref, intent = _oracle_outcome(O, s, O.DEC_REFERENCE), _oracle_outcome(O, s, O.DEC_STRIDE)
            if kind == "run_past_n":
                assert isinstance(ref, Exception) and isinstance(intent, Exception), (kind, seed)
            elif kind == "digit_at_n":
                assert isinstance(ref, Exception) and not isinstance(intent, Exception), (kind, seed)
            else:
                assert not isinstance(ref, Exception) and np.array_equal(ref, intent), (kind, seed)
        assert in_head == {True, False}, (kind, in_head)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", END_KINDS)
def test_end_rules_in_heads(nice, O, opts, kind):
    """Strict and default mode on the crafted ends, with 1024-bit slices: the
    oracle's outcome (failure, or its pixels), and the status the decoder
    gives when dec_emit parses every slice (no events kept)."""
    for seed in END_SEEDS:
        s, _ = _crafted_end(O, seed, kind)
        for flags, omode in ((nice.DEC_STRICT_REFERENCE, O.DEC_REFERENCE), (nice.DEC_ALPHA_FILL_FF, O.DEC_STRIDE)):
            want = _oracle_outcome(O, s, omode)
            got = {}
            for path in ("events", "no_events"):
                opts.reset()
                opts.setenv("NICE_DEC_SLICE_BITS", 1024)
                if path == "no_events":
                    opts.setenv("NICE_DEC_NO_EVENTS", 1)
                try:
                    got[path] = np.frombuffer(nice.decode_bytes(s, flags)[0], np.uint8)
                except nice.NiceError as e:
                    got[path] = e
            g = got["events"]
            if isinstance(want, Exception):
                assert isinstance(g, Exception), (kind, seed, flags)
                assert isinstance(got["no_events"], Exception) and g.code == got["no_events"].code == nice.E_FORMAT, \
                    (kind, seed, flags, g, got["no_events"])
            else:
                assert not isinstance(g, Exception), (kind, seed, flags, g)
                assert np.array_equal(g, want) and np.array_equal(got["no_events"], want), (kind, seed, flags)
