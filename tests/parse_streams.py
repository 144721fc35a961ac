"""The hand-built streams of tests/test_parse_streams_cpu.py (what they hold)
and tests/test_parse_paths.py (what the GPU decodes from them): one table
profile of crafted_streams.make_stream each, uniformly drawn modes and
references, short runs with trailing zero digits, and with `long_p` pixels of
their streams' longest codes.

Every profile has streams of 515x16 pixels (8240 pixels, over 128 slices of
1024 bits: more than one wave of slices) and one of 67x16 (fewer than 64
slices: a single wave).  Each stream is built and decoded by the oracle once.
"""
import functools

import numpy as np

import crafted_streams as C

H = 16
W_MAIN, W_SMALL = 515, 67
# profile -> (what make_stream gets, the parse dec_tables must choose, the streams with long codes)
PROFILES = {
    "flat": (dict(long_p=0.0), True, []),
    "long_event": (dict(long_p=0.06), True, []),
    "all12": (dict(long_p=0.06), False, [0, 1, 2, 3, 5, 6, 7, 8]),
}
# (width, seed) per profile: seeds at which tests/test_parse_streams_cpu.py's
# conditions hold.  A 67x16 stream has some 20 slices of 1024 bits and 5 of
# 4096, and flat codes re-synchronise slowly, so at many seeds no re-parse
# meets the previous parse inside its slice and no head is placed (the same
# slices on either parse: it is a property of the bits); these seeds have
# re-parses that meet at both slice sizes
STREAMS = {
    "flat": [(W_MAIN, 5), (W_MAIN, 7), (W_SMALL, 11)],
    "long_event": [(W_MAIN, 29), (W_MAIN, 2), (W_SMALL, 11)],
    "all12": [(W_MAIN, 29), (W_MAIN, 1), (W_SMALL, 10)],
}
SLICES = [1024, 4096]


def n_slices(s, slice_bits):
    return -(-(len(s) * 8 - C.DATA_START_BITS) // slice_bits)


@functools.lru_cache(maxsize=None)
def stream(profile, W, seed):
    """(stream, make_stream's info, the oracle's reference decode, its intent decode)."""
    from conftest import oracle_mod
    O = oracle_mod()
    s, info = C.make_stream(O, 1000 * W + seed, W=W, H=H, uniform=True, run_p=0.03, run_max=9,
                            tables=profile, **PROFILES[profile][0])
    ref, dims = O.decode(s)
    assert dims == (W, H, 3)
    intent = O.decode(s, O.DEC_STRIDE)[0]
    ref.setflags(write=False)
    intent.setflags(write=False)
    return s, info, ref, intent


def maxes(s):
    """The ten table maxima a stream's header states."""
    return [mx for mx, _ in C.header_lengths(s)]


OPT_DEC_HEV_CAP = 15          # include/nice_test.h: NICE_OPT_DEC_HEV_CAP


def head_stats(err):
    """The 'slice heads' line of the decoder's statistics as a dict."""
    line = [l for l in err.splitlines() if "slice heads:" in l][-1]
    body = line.split("slice heads:")[1].split("(")[0]
    return {k: int(v) for k, v in (kv.split("=") for kv in body.split())}


def sync_flags(err):
    """The sync-flags line: (flags of the queued iterations, settle, final; queued)."""
    line = [l for l in err.splitlines() if "sync iterations that changed an entry" in l][-1]
    flags = [int(x) for x in line.split(":")[1].split("(")[0].split()]
    return flags, int(line.split("(queued")[1].split(",")[0])


def tolerant_maxes(s):
    """The table maxima the decoder works with under DEC_TOLERANT_HEADER, from
    the header's lengths alone (dec_tables' repair of spilled max fields,
    SURVEY.md A.5): from the last stream down, a stream whose longest length
    mx is 32 or more took mx >> 5 out of the low p bits of the previous
    stream's last length (p: table-header bits before it, mod 8); its max is
    its longest length of at most 31 bits."""
    lens = [l.astype(np.int64) for _, l in C.header_lengths(s)]
    out = [0] * 10
    for st in range(9, -1, -1):
        mx = int(lens[st].max())
        out[st] = int(lens[st][lens[st] <= 31].max())
        if mx >= 32 and st > 0:
            pm = (1 << (sum(5 + 7 * n for n in C.SIZES[:st]) & 7)) - 1
            last = int(lens[st - 1][-1])
            lens[st - 1][-1] = (last & ~pm) | ((last - (mx >> 5)) & pm)
    return out


def parse_stats(err):
    """The 'parse' line of the decoder's statistics: frames, fast, slow_parse
    as numbers, max and lut_bits as lists."""
    line = [l for l in err.splitlines() if "[nice dec stats] parse:" in l][-1]
    kv = dict(f.split("=") for f in line.split("parse:")[1].split() if "=" in f)
    return {k: [int(x) for x in v.split(",")] if k in ("max", "lut_bits") else int(v) for k, v in kv.items()}
