"""The inputs of tests/test_parse_paths.py hold what they are for (no GPU).

dec_tables picks one of two parses per frame: the fast parse (one 64-bit
window per pixel event, every symbol one first-level lookup) when no code is
longer than its first-level table and the longest event fits 64 bits, the
general parse (symbol by symbol, long-code search) otherwise.
crafted_streams.lut_plan restates that decision; the table profiles of
crafted_streams.make_stream put hand-built content (back reference 0,
references a lower index would match as well, trailing zero digits, uniform
modes) on either parse.  These are conditions on the input; they are checked
here, pooled over each profile's streams, not on the GPU.
"""
import hashlib

import numpy as np
import pytest

import crafted_streams as C
import parse_streams as PS


def test_lut_plan_tie_case_and_largest_fast_set():
    """Fourteen shrinks through ties, the first of equally wide tables losing
    its bit; and the largest table set that stays within the budget."""
    assert C.lut_constants() == (12, 12288)   # the figures below are worked out for these
    lut_bits, long_streams, longest, fast = C.lut_plan([12, 12, 12, 12, 10, 12, 12, 12, 12, 10])
    assert lut_bits == [10, 10, 10, 10, 10, 10, 10, 11, 11, 10]
    assert sum(12 - b for b in lut_bits[:4] + lut_bits[5:9]) == 14
    assert long_streams == [0, 1, 2, 3, 5, 6, 7, 8] and not fast
    # the tie order shows in these widths: were the last of equally wide
    # tables to shrink first, streams 7 and 8 would end at 10 bits and 0 and 1
    # at 11, and the GPU cases of this shape compare the reported widths
    last = [12, 12, 12, 12, 10, 12, 12, 12, 12, 10]
    while sum(1 << b for b in last) > 12288:
        last[max(range(10), key=lambda st: (last[st], st))] -= 1
    assert last == [11, 11, 10, 10, 10, 10, 10, 10, 10, 10] != lut_bits
    lut_bits, long_streams, longest, fast = C.lut_plan([8, 12, 11, 12, 10, 9, 6, 5, 5, 4])
    assert lut_bits == [8, 12, 11, 12, 10, 9, 6, 5, 5, 4] and sum(1 << b for b in lut_bits) == 12176
    assert long_streams == [] and longest == 12 + 10 + 11 + 2 * 12 == 57 and fast
    # one more bit anywhere in that set is over the budget: the first widest table shrinks
    assert C.lut_plan([9, 12, 11, 12, 10, 9, 6, 5, 5, 4])[:2] == ([9, 11, 11, 12, 10, 9, 6, 5, 5, 4], [1])
    # a code over the width cap is a long code whatever the budget
    assert C.lut_plan([13, 4, 4, 4, 4, 4, 4, 4, 4, 4])[:2] == ([12, 4, 4, 4, 4, 4, 4, 4, 4, 4], [0])


def test_default_streams_are_unchanged(O):
    """make_stream's defaults draw what they always drew: the corpus of
    tests/test_strict_refill.py (its seeds' streams, concatenated).  This
    hash was taken when the table profiles went in, after comparing the
    streams of all 160 seeds byte for byte with those of the generator before
    them.  It is not the `7dc779e2...` an earlier commit message quotes for
    the same corpus: how that one was computed is not recorded, and neither
    the concatenation nor a hash of the per-stream digests reproduces it."""
    h = hashlib.sha256()
    for seed in range(160):
        h.update(C.make_stream(O, seed)[0])
    assert h.hexdigest() == "5062afc0861570dc764f55ed0de00460e2f6811a97d69119aebf7894460c4674"


def test_existing_hand_built_streams_take_the_general_parse(O):
    """Why the profiles exist: make_stream's default tables (counts in 1..60)
    have long codes, so test_ref_streams, test_strict_refill and the slow-sync
    stream run on the general parse; the slow-sync variant with a flat
    SMALL_DIFF table is fast."""
    for s in (C.make_stream(O, 515001, W=515, H=16, deep=C.NO_DEEP, uniform=True)[0], C.make_stream(O, 3)[0],
              C.make_slow_sync(O, 5, 64, 64)):
        assert not C.lut_plan(PS.maxes(s))[3]
    assert C.lut_plan(PS.maxes(C.make_slow_sync(O, 5, 64, 64, flat_small_diff=True)))[3]


def test_encoded_frames_small_ones_general_512_fast(O):
    """The SYN-v1 frames of tests/test_head_events.py have long codes in
    SMALL_DIFF and LUMA2_BASE; the 512x512 frame of tests/test_parse_paths.py
    has none."""
    from test_head_events import SHAPES
    for w, h, c in SHAPES:
        s = O.encode(O.gen_syn_v1(w, h, c, 1), w, h, c)
        assert C.lut_plan(PS.maxes(s))[1::2] == ([5, 6], False), (w, h, c)
    s = O.encode(O.gen_syn_v1(512, 512, 4, 1), 512, 512, 4)
    assert C.lut_plan(PS.maxes(s))[1::2] == ([], True)


@pytest.mark.parametrize("profile", PS.PROFILES)
def test_profile_takes_its_parse_and_the_oracle_decodes_it(profile):
    _, want_fast, want_long = PS.PROFILES[profile]
    for W, seed in PS.STREAMS[profile]:
        s, info, ref, intent = PS.stream(profile, W, seed)
        hdr = C.header_lengths(s)
        for st, (mx, lens) in enumerate(hdr):
            assert mx == lens.max() and np.array_equal(lens, info["lens"][st])
        lut_bits, long_streams, longest, fast = C.lut_plan(PS.maxes(s))
        assert (fast, long_streams) == (want_fast, want_long), (W, seed, PS.maxes(s), lut_bits)
        assert max(PS.maxes(s)) <= 12     # the reference's reader finishes
        assert np.array_equal(ref, intent), (W, seed)
    assert {"flat": [8, 4, 6, 5, 4, 9, 6, 5, 5, 4], "long_event": [8, 12, 11, 12, 10, 9, 6, 5, 5, 4],
            "all12": [12, 12, 12, 12, 10, 12, 12, 12, 12, 10]}[profile] == PS.maxes(s)


@pytest.mark.parametrize("profile", PS.PROFILES)
def test_slices(profile):
    """The 515x16 streams have more than a wave of slices, one of them a count
    that is no multiple of 64; the 67x16 stream fits a single wave."""
    counts = []
    for W, seed in PS.STREAMS[profile]:
        n = PS.n_slices(PS.stream(profile, W, seed)[0], 1024)
        assert (n >= 128) if W == PS.W_MAIN else (n < 64), (W, seed, n)
        counts.append(n)
    assert any(n % 64 for W, n in zip(PS.STREAMS[profile], counts) if W[0] == PS.W_MAIN), counts


@pytest.mark.parametrize("profile", ["flat", "long_event"])
def test_fast_profiles_hold_what_no_encoder_writes(profile):
    seen, digits, col0, zero_tail, run_at_end = set(), set(), 0, 0, 0
    for W, seed in PS.STREAMS[profile]:
        _, info, _, _ = PS.stream(profile, W, seed)
        for p, what in enumerate(info["pixels"]):
            if what is not None:
                seen.add(what)
                col0 += what == (0, 0) and p % W == 0
        run_at_end += info["pixels"][-1] is None
        pfx = [syms[0][1] for _, _, syms in info["events"][:-1]]   # without the extra prefix at the end
        digits |= {v for v in pfx if v >= 5}
        zero_tail += sum(1 for a, b in zip(pfx, pfx[1:]) if a >= 5 and b == 5)
    assert {m for m, _ in seen} == set(range(5))
    assert {k for m, k in seen if m == 0} == set(range(5)) and col0 >= 1
    assert {k for m, k in seen if m == 2} == set(range(11))
    assert digits == set(range(5, 13)) and zero_tail >= 1
    assert run_at_end >= 1


def test_long_event_streams_hold_the_longest_event_everywhere():
    """An event of the model's longest_event_bits at every bit alignment of
    its start (the fast parse shifts three ring words by it), and across a
    slice end at both slice sizes."""
    align, across = set(), {b: 0 for b in PS.SLICES}
    for W, seed in PS.STREAMS["long_event"]:
        s, info, _, _ = PS.stream("long_event", W, seed)
        longest = C.lut_plan(PS.maxes(s))[2]
        assert 56 <= longest <= 64
        assert max(n for _, n, _ in info["events"]) == longest
        # events that need the third ring word of the fast window (start bit
        # within its word + length over 64): in every stream on its own, many
        # of the longest, so that a settle walk (test_settle_walks_the_fast_parse)
        # meets one wherever its ring happens to end
        third = [n for pos, n, _ in info["events"] if (C.DATA_START_BITS + pos) % 32 + n > 64]
        assert third.count(longest) >= (40 if W == PS.W_MAIN else 8), (W, seed, len(third))
        for pos, n, _ in info["events"]:
            if n == longest:
                align.add((C.DATA_START_BITS + pos) % 32)
                for b in PS.SLICES:
                    across[b] += pos // b != (pos + n - 1) // b   # a slice end strictly inside it
    assert align == set(range(32)), sorted(set(range(32)) - align)
    assert min(across.values()) >= 1, across


def test_all12_streams_read_long_codes_in_eight_streams():
    """Every stream with codes over its first-level width has them read at
    least 20 times; the prefix stream both for a coded mode and a run digit."""
    reads = {st: 0 for st in PS.PROFILES["all12"][2]}
    pfx_mode = pfx_digit = 0
    for W, seed in PS.STREAMS["all12"]:
        s, info, _, _ = PS.stream("all12", W, seed)
        lut_bits = C.lut_plan(PS.maxes(s))[0]
        for _, _, syms in info["events"]:
            for st, v, n in syms:
                if n > lut_bits[st]:
                    reads[st] += 1
                    pfx_mode += st == 1 and v < 5
                    pfx_digit += st == 1 and v >= 5
    assert min(reads.values()) >= 20, reads
    assert pfx_mode >= 20 and pfx_digit >= 20, (pfx_mode, pfx_digit)
