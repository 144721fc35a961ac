"""Host model of the row reconstructor's LDS ring addressing (dec_rows_body,
csrc/nice_rows.hip): the table-form pre-pass reads a reference of record
class c at word 4 + slot(y - rows_c) * RS + 17 * lane + d + (d >> 4),
d = p - px_c, with no wrap logic, because every emitted row also writes two
halos -- lane 0 its first three pixels past the end of the row above (row 0
too: ring row -1), the last lane its last three pixels before the start of the
next slot.  The index counts from the ring's first word (the table entries
carry the four left halo words), so it is never negative, and every launched
lane forms one for each of its 16 pixels whatever the class: the idle lanes of
the last wave, whose own words would lie past the ring, use lane 0's.
tests/test_rows_host.py proves the same of the kernel text itself under
AddressSanitizer; this states it as arithmetic.  This replays
the kernel's stores for whole frames and checks that every reference the
reference codec can make (code.rs:141-145 offsets: rows 1..3 back, -3..3
pixels) reads the pixel the raster says, except the ones into the current row
(W_CUR, patched by the last lane).  CPU only: it pins the index arithmetic.
"""
import numpy as np
import pytest

# record classes 4..13 -> (rows back, pixels back), as cls_rows / cls_px
UP_CLASSES = {4: (1, 0), 5: (1, -1), 6: (2, 0), 7: (1, -3), 8: (3, -1), 9: (3, 0),
              10: (3, 1), 11: (1, 3), 12: (3, 3), 13: (3, -3)}
RB = 4


def g(x):
    return x + (x >> 4)   # Python >> on ints is arithmetic, as the kernel's int shift


def ring_stride(w):
    return w + (w >> 4) + 24


# record class -> pixels back + 3 (classes 0..3: the pixel itself and 1..3 back, no rows)
DXP3 = {0: 3, 1: 4, 2: 5, 3: 6, **{c: px + 3 for c, (_, px) in UP_CLASSES.items()}}
ROWS = {0: 0, 1: 0, 2: 0, 3: 0, **{c: rows for c, (rows, _) in UP_CLASSES.items()}}


def table_index(w, y, c, lane, p, active):
    """The word, from the ring's first one, that a lane's pre-pass loads for pixel p of class c on row y."""
    off = RB + ((y - ROWS[c]) & 3) * ring_stride(w) + 3 - DXP3[c]   # rtab[.][c].y
    ad = (17 * lane if active else 0) + off
    if p < 3 or p > 12:
        ad += (p + 3 - DXP3[c]) >> 4                                  # padding word crossed
    return ad + p


def replay(w, rows_to_emit, img):
    """Ring words after emitting rows 0..rows_to_emit-1 (value = pixel id + 1)."""
    rs = ring_stride(w)
    ring = np.zeros(4 * rs + RB, dtype=np.int64)
    nseg = (w + 15) // 16
    for y in range(rows_to_emit):
        base = RB + (y & 3) * rs
        for lane in range(nseg):
            x0 = 16 * lane
            nvalid = min(16, w - x0)
            for p in range(16):   # padding pixels (p >= nvalid) land in the spare words
                val = img[y, x0 + p] if p < nvalid else img[y, x0 + nvalid - 1]
                ring[base + x0 + (x0 >> 4) + p] = val
        hb = RB + ((y - 1) & 3) * rs   # lane 0: row y-1's right halo (row 0: ring row -1)
        for k in range(3):
            ring[hb + g(w + k)] = img[y, k]
        nb = RB + ((y + 1) & 3) * rs   # last lane: row y+1's left halo
        for x in range(w - 3, w):
            ring[nb + (x - w) - 1] = img[y, x]
    return ring


@pytest.mark.parametrize("w", [64, 100, 1000, 3840])
def test_table_form_reads_match_raster(w):
    h = 9
    img = (np.arange(h * w, dtype=np.int64) + 1).reshape(h, w)
    rs = ring_stride(w)
    nseg = (w + 15) // 16
    for y in range(2, h):   # row 2: the references to pixels 0..2 through ring row -1's right halo
        ring = replay(w, y, img)   # the ring as row y's pre-pass sees it
        checked = 0
        for c, (rows, px) in UP_CLASSES.items():
            for lane in range(nseg):
                for p in range(min(16, w - 16 * lane)):
                    x = 16 * lane + p
                    if y * w + x < rows * w + px:            # the offset is not valid yet
                        continue
                    got = ring[table_index(w, y, c, lane, p, True)]
                    i = y * w + x - (rows * w + px)          # the raster reference
                    tx = x - px
                    if rows == 1 and tx >= w:                # into row y itself: W_CUR
                        assert lane == nseg - 1
                        continue
                    assert got == img.flat[i], (w, y, c, lane, p)
                    checked += 1
        assert checked > 0


@pytest.mark.parametrize("w", [64, 66, 67, 100, 1000, 1026, 1600, 3840, 8193, 8194, 8208, 8211, 16384])
def test_every_launched_lane_stays_inside_the_ring(w):
    """Every index that any launched lane forms -- idle lanes and padding
    pixels included, every class (the load is unconditional) -- lies inside the
    4 * ring_stride words the planner allocates (rows_lds_bytes, DecPlan::rowbuf;
    the four halo words before pixel 0 are the first slot's own)."""
    nseg = (w + 15) // 16
    threads = (nseg + 63) // 64 * 64
    words = 4 * ring_stride(w)   # the allocation; the model's own array has RB more
    lo, hi = words, -1
    for y in range(4):   # the index depends on y through the slot only
        for c in DXP3:
            for lane in range(threads):
                for p in range(16):
                    i = table_index(w, y, c, lane, p, lane < nseg)
                    assert 0 <= i < words, (w, y, c, lane, p, i)
                    lo, hi = min(lo, i), max(hi, i)
    assert lo == 0   # lane 0, pixel 0, three pixels back in slot 0: the first halo word
    # the form this replaced: idle lanes with their own base, the index relative to pixel 0 as uint32
    old = lambda y, c, lane, p: (table_index(w, y, c, lane, p, True) - RB) % 2**32 + RB
    assert old(0, 3, 0, 0) >= words
    if threads - nseg >= 3:   # class 4 on row 0 reads slot 3, the ring's last
        assert old(0, 4, threads - 1, 15) >= words


def test_ring_fits_two_blocks_per_cu_at_4k():
    # dec_rows at 3840 columns: 256 lanes, tails + ring must leave two blocks per CU
    w, thr = 3840, 256
    lds = (thr * 7 + 8 + 4 * ring_stride(w)) * 4 + 384    # + static (class table, rtab)
    assert 2 * lds <= 160 * 1024
