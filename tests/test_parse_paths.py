"""The same pixels from both parses, and the parse each stream is meant for.

dec_tables gives a frame the fast parse (DecTables::fast: one 64-bit window
per pixel event, pixel_event_fast / pixel_event_fast_at, every symbol one
first-level lookup) or the general parse (dsym_gp: symbol by symbol, ring
top-up, long-code search); dec_sync, dec_sync_settle and dec_emit have a loop
for each (dec_strict_refill: the general one only).  The hand-built streams
of tests/parse_streams.py put what no encoder writes on the fast parse
("flat"), its longest events at every bit alignment and across slice ends
("long_event"), and long codes into eight streams of the general parse, the
prefix stream included ("all12"); tests/test_parse_streams_cpu.py checks that
they hold it.

Which fast code a case reaches: dec_sync and dec_emit parse with
pixel_event_fast_at in a relative-position loop each (own refill bound), and
have no other fast loop; pixel_event_fast and lane_ok_fast run in
dec_sync_settle only, which walks slices when the queued iterations did not
reach the fixpoint -- test_settle_walks_the_fast_parse (one queued iteration)
and the slow-sync stream.

Every case decodes one small stream, compares every byte with the oracle's
decode in the default mode and with DEC_STRICT_REFERENCE, and asserts from the
statistics which parse ran: crafted_streams.lut_plan must give the reported
`fast` and `lut_bits`, so a case on another parse than it names fails.
"""
import numpy as np
import pytest

import crafted_streams as C
import parse_streams as PS

pytestmark = pytest.mark.gpu

from parse_streams import OPT_DEC_HEV_CAP, head_stats as _head_stats

MODES = ["default", "slow_parse", "no_events", "small_hev"]
CASES = [(p, W, seed) for p in PS.PROFILES for W, seed in PS.STREAMS[p]]


def _set_mode(opts, slice_bits, mode):
    opts.setenv("NICE_DEC_SLICE_BITS", slice_bits)
    opts.setenv("NICE_DEC_STATS", 1)
    if mode == "slow_parse":
        opts.setenv("NICE_DEC_SLOW_PARSE", 1)
    if mode == "no_events":
        opts.setenv("NICE_DEC_NO_EVENTS", 1)
    if mode == "small_hev":
        assert opts.L.nice_test_set_option(OPT_DEC_HEV_CAP, 4) == 0


def _check_stats(err, s, slice_bits, mode, frames=1):
    """The parse that ran is the one the model gives the header's tables, the
    slice heads are accounted for and none ended off its meeting point."""
    lut_bits, _, _, fast = C.lut_plan(PS.maxes(s))
    ps = PS.parse_stats(err)
    print(ps)
    assert ps["max"] == PS.maxes(s)
    assert ps["lut_bits"] == lut_bits, (ps, lut_bits)
    assert (ps["frames"], ps["fast"]) == (frames, frames if fast else 0), (ps, fast)
    assert ps["slow_parse"] == (1 if mode == "slow_parse" else 0), ps
    st = _head_stats(err)
    print(st)
    assert st["invariant_violations"] == 0
    counted = sum(st[k] for k in ("none", "placed", "emitted", "whole_slice_emitted"))
    if mode == "no_events":
        # dec_place counts the heads, and without the first pass's events it
        # does not run: dec_emit parses every slice and nothing is counted
        assert counted == 0, st
    else:
        assert counted == PS.n_slices(s, slice_bits), st
    if mode == "small_hev":
        assert st["placed"] == 0, st      # an event is at most 64 bits, a head at least 512: none fits 4 events
    elif mode != "no_events":
        assert st["placed"] > 0, st
    return fast


def _first_difference(got, want, W, info=None):
    p = int(np.nonzero(got != want)[0][0]) // 3
    what = ""
    if info is not None:
        what = f", written as {info['pixels'][p]}"
    return f"first differing pixel {p} (row {p // W}, column {p % W}){what}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("slice_bits", PS.SLICES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx16-s%d" % c)
def test_crafted_stream(nice, opts, capfd, case, slice_bits, mode):
    """profile x stream x slice size x {both parses, every slice parsed by
    dec_emit, every head overflowing its buffer}, default and strict mode:
    the reference's pixels (its reader finishes on tables of at most 12 bits,
    and its decode equals the intent decode, checked without a GPU)."""
    profile, W, seed = case
    s, info, ref, _ = PS.stream(profile, W, seed)
    _set_mode(opts, slice_bits, mode)
    for flags in (0, nice.DEC_STRICT_REFERENCE):
        got = np.frombuffer(nice.decode_bytes(s, flags=flags)[0], np.uint8)
        fast = _check_stats(capfd.readouterr().err, s, slice_bits, mode)
        assert fast == PS.PROFILES[profile][1]
        if not np.array_equal(got, ref):
            pytest.fail(f"flags {flags}: " + _first_difference(got, ref, W, info))


FAST_CASES = [c for c in CASES if PS.PROFILES[c[0]][1]]


@pytest.mark.parametrize("slice_bits", PS.SLICES)
@pytest.mark.parametrize("case", FAST_CASES, ids=lambda c: "%s-%dx16-s%d" % c)
def test_settle_walks_the_fast_parse(nice, opts, capfd, case, slice_bits):
    """dec_sync_settle's fast code: the only user of pixel_event_fast and
    lane_ok_fast at these sizes (dec_sync takes the relative-position loop,
    pixel_event_fast_at with its own refill bound; dec_emit has the general
    parse only).  With one queued iteration (NICE_DEC_SYNC_QUEUED=1) the
    slices are not at their fixpoint when the settle starts, so it walks them
    event by event: on the long_event streams through 57-bit events at every
    bit alignment, with a ring refill once no third word is left.  The settle
    must have run, the final pass must move nothing (a settle that parsed an
    event wrongly leaves an entry the final dec_sync moves, and the frame
    fails), and every byte must be the reference's, in default and strict
    mode."""
    profile, W, seed = case
    s, info, ref, _ = PS.stream(profile, W, seed)
    _set_mode(opts, slice_bits, "default")
    opts.setenv("NICE_DEC_SYNC_QUEUED", 1)
    for flags in (0, nice.DEC_STRICT_REFERENCE):
        got = np.frombuffer(nice.decode_bytes(s, flags=flags)[0], np.uint8)
        err = capfd.readouterr().err
        assert _check_stats(err, s, slice_bits, "default")
        moved, queued = PS.sync_flags(err)
        print(moved, queued)
        assert queued == 1 and moved[0] == 1 and moved[16] == 1 and moved[17] == 0, (moved, queued)
        if not np.array_equal(got, ref):
            pytest.fail(f"flags {flags}: " + _first_difference(got, ref, W, info))


_syn_cache = {}


def _syn512(O):
    if not _syn_cache:
        w, h, c = 512, 512, 4
        s = O.encode(O.gen_syn_v1(w, h, c, 1), w, h, c)
        want = O.decode(s, O.DEC_STRIDE)[0].reshape(-1, c)[:, :3].copy()
        want.setflags(write=False)
        # the reference's own decode exists for three channels only: the same
        # stream with header byte 12 = 3, for the strict mode
        s3 = s[:12] + bytes([3]) + s[13:]
        ref3 = O.decode(s3)[0]
        ref3.setflags(write=False)
        assert np.array_equal(ref3.reshape(-1, 3), want)
        _syn_cache["syn"] = (s, want, s3, ref3)
    return _syn_cache["syn"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("slice_bits", PS.SLICES)
def test_smallest_fast_syn_frame(nice, O, opts, capfd, slice_bits, mode):
    """syn512x512x4: the smallest SYN-v1 frame of tests/test_head_events.py's
    kind whose tables are fast (its 256x256 and 257x130 frames have long
    codes in SMALL_DIFF and LUMA2_BASE): encoder-written content on the fast
    parse, the kept head events and dec_place's head-then-tail walk fed by
    the fast relative-position loop, at forced slice sizes.  Default mode on
    the RGBA stream; DEC_STRICT_REFERENCE on its three-channel form (the same
    bits with header byte 12 = 3), which the reference's decoder reads."""
    s, want, s3, ref3 = _syn512(O)
    assert C.lut_plan(PS.maxes(s))[3]
    _set_mode(opts, slice_bits, mode)
    got = np.frombuffer(nice.decode_bytes(s)[0], np.uint8).reshape(-1, 4)[:, :3]
    assert _check_stats(capfd.readouterr().err, s, slice_bits, mode)
    assert np.array_equal(got, want)
    got = np.frombuffer(nice.decode_bytes(s3, flags=nice.DEC_STRICT_REFERENCE)[0], np.uint8)
    assert _check_stats(capfd.readouterr().err, s3, slice_bits, mode)
    assert np.array_equal(got, ref3)


SLOW_SYNC_SEED = 5   # tests/test_async_decode.py::test_settle_slow_sync_stream's


def test_slow_sync_stream_on_the_fast_parse(nice, O, opts, capfd):
    """crafted_streams.make_slow_sync with a flat SMALL_DIFF table, at the
    size of test_settle_slow_sync_stream and with 1024-bit slices: exact on
    the fast parse, through more Jacobi iterations than are queued (the last
    queued one still moved an entry, the settle moved, the final pass did
    not), which is dec_sync_settle's fast code."""
    W, H = 512, 512
    s = C.make_slow_sync(O, SLOW_SYNC_SEED, W, H, flat_small_diff=True)
    ref = O.decode(s)[0]
    _set_mode(opts, 1024, "default")
    got = np.frombuffer(nice.decode_bytes(s)[0], np.uint8)
    err = capfd.readouterr().err
    assert np.array_equal(got, ref)
    ps = PS.parse_stats(err)
    assert ps["fast"] == 1 and ps["slow_parse"] == 0 and ps["lut_bits"] == C.lut_plan(PS.maxes(s))[0], ps
    assert _head_stats(err)["invariant_violations"] == 0
    line = [l for l in err.splitlines() if "sync iterations that changed an entry" in l][-1]
    print(line)
    flags = [int(x) for x in line.split(":")[1].split("(")[0].split()]
    queued = int(line.split("(queued")[1].split(",")[0])
    assert flags[queued - 1] == 1 and flags[16] == 1 and flags[17] == 0, line
