"""Planted-reference frames (test input; CPU only, numpy).

The codec's 16 reference offsets (csrc/nice_format.h: five back references,
eleven luma references, up to three rows and +-3 pixels away) are addressed by
every classify kernel and every row kernel in its own way.  `planted_frame`
builds frames in which chosen pixels are MADE to take a chosen reference at
the positions where those kernels differ: the row's first and last columns,
tile, segment, wave and strip edges, a block's first pixels, the first pixel
at which an offset is valid.

A CELL is (kind, class, arg): kind ("B", k) for back reference k = 1..4 or
("L", k) for luma reference k = 0..10 (back reference 0 cannot be emitted: a
pixel equal to its left neighbour is a run member), and a position class

  a  column == arg                          (0..3, W-4..W-1)
  b  p mod 1024 == arg                      (0..3, 1020..1023: the encoder's tiles)
  c  p == off_k                             (references pixel 0: the first valid position)
  d  max(arg, off_k) <= p < arg + off_k     (arg a block or band start: the reference lies before it)
  e  column mod 2048 == arg                 (the strip kernel's strips)
  f  column mod 16 == arg                   (the row kernels' segments, pooled)
  g  column == arg                          (e-3..e+2 around a wave or strip edge e)

The generator plants each cell a few times at random positions of its class.
The encoder takes the first match of back references 0..4, small diff, luma2,
luma 0..10, so a planting can be shadowed; the generator only draws a shadowed
luma delta again, as a hint.  `coverage` counts, from the oracle's trace
(O.encode_trace), what each cell really got, and the tests assert on that.

Some cells of classes c and d exclude each other in one frame (C_LEFT_OUT,
D_LEFT_OUT), so every shape has three frames, `variant` 0..2, each leaving
out the cells it cannot hold; the three tables together hold every cell.
"""
import functools
import heapq

import numpy as np

TILE = 1024
BLOCK = 16 * TILE
BACK_OFF = lambda W: [1, W, W - 1, 2, 2 * W]
LUMA_OFF = lambda W: [1, W, W - 1, W - 3, 3, 3 * W - 1, 3 * W, 3 * W + 1, W + 3, 3 * W + 3, 3 * W - 3]
KINDS = [("B", k) for k in range(1, 5)] + [("L", k) for k in range(11)]
# O.encode_trace's byte for a kind (mode << 4 | k; modes: 0 back reference, 2 luma)
CODE = lambda kind: (0 if kind[0] == "B" else 2) << 4 | kind[1]
REPEATS = 3      # plantings per cell
SPRINKLE = 200   # one random planting per this many pixels


def offset(kind, W):
    return (BACK_OFF(W) if kind[0] == "B" else LUMA_OFF(W))[kind[1]]


def band_starts(W, H, R):
    """First pixel of bands 1..R-1 (sharded.band_tiles: contiguous tile ranges)."""
    n_tiles = (W * H + TILE - 1) // TILE
    return [n_tiles * r // R * TILE for r in range(1, R)]


def strip_edges(W, strips):
    """Columns where dec_rows_split's strips meet: sps * 16 * j, sps the
    segments per strip as plan_decode computes them."""
    nseg = (W + 15) // 16
    sps = (nseg + strips - 1) // strips
    return [sps * 16 * j for j in range(1, strips) if sps * 16 * j < W]


def wave_edges(W, seg=16):
    """Columns where the row kernels' waves meet (64 lanes of one segment each)."""
    return list(range(64 * seg, W, 64 * seg))


# class c: every such pixel references pixel 0, so a back reference there (a copy
# of pixel 0) shadows others: pixel 2 as back reference 3 makes luma reference 0
# predict pixel 3 as well as luma reference 4 does, pixel W as back reference 1
# takes pixel 2W from back reference 4, pixel W-1 as back reference 2 makes pixel W
# a run member.  Variant 0 holds the luma references' cells, variants 1 and 2 the
# back references'.  Class d: pixel B can only be luma reference 0, which leaves
# pixel B+1 to back reference 3, and then luma reference 0 predicts B+2 as well as
# luma reference 4 does: variant 0 leaves out back reference 3's cells, the others
# luma reference 4's.
_LUMA = {("L", k) for k in range(11)}
C_LEFT_OUT = ({("B", k) for k in range(1, 5)}, _LUMA | {("B", 2), ("B", 4)}, _LUMA | {("B", 1)})
D_LEFT_OUT = ({("B", 3)}, {("L", 4)}, {("L", 4)})
VARIANTS = range(3)


def cell_table(W, H, variant, starts=(), strip=False, decoder=False, edges=()):
    """The cells of one frame.  starts: block and band starts (class d);
    strip: add class e; decoder: add class f; edges: wave and strip edges
    (class g).  Class b (15 kinds on the pixels at one in-tile offset) is
    counted from 24 tiles up."""
    N = W * H
    cells = []
    for kind in KINDS:
        off = offset(kind, W)
        for x in sorted({0, 1, 2, 3, W - 4, W - 3, W - 2, W - 1}):
            cells.append((kind, "a", x))
        if N // TILE >= 24:
            for t in (0, 1, 2, 3, 1020, 1021, 1022, 1023):
                cells.append((kind, "b", t))
        if kind not in C_LEFT_OUT[variant]:
            cells.append((kind, "c", off))
        for B in starts:
            assert 0 < B < N, B
            if kind not in D_LEFT_OUT[variant]:
                cells.append((kind, "d", B))
        if strip:
            for t in (0, 1, 2, 2045, 2046, 2047):
                cells.append((kind, "e", t))
        if decoder:
            for t in (0, 1, 2, 13, 14, 15):
                cells.append((kind, "f", t))
        for e in edges:
            for x in range(e - 3, min(e + 3, W)):
                cells.append((kind, "g", x))
    return cells


def _candidates(cell, W, H, rng):
    """(how many positions the cell's class has where its offset is valid, a
    few of them at random: all of them where they are few)."""
    kind, cls, arg = cell
    off = offset(kind, W)
    N = W * H
    if cls == "c":
        return 1, [arg]
    if cls == "d":
        lo, hi = max(arg, off), min(arg + off, N)
        return hi - lo, [lo + int(i) for i in (rng.permutation(hi - lo) if hi - lo <= 16 else rng.integers(0, hi - lo, 16))]
    if cls == "b":
        first = -(-(off - arg) // TILE) if off > arg else 0
        last = (N - 1 - arg) // TILE
        return max(0, last + 1 - first), [arg + TILE * int(m) for m in rng.permutation(np.arange(first, last + 1))[:64]]
    y0 = -(-off // W)   # every column of row y0 is at or past the offset
    if y0 >= H:
        return 0, []
    if cls in ("a", "g"):
        return H - y0, [int(y) * W + arg for y in rng.permutation(np.arange(y0, H))]
    xs = np.arange(arg, W, 2048 if cls == "e" else 16)
    if xs.size == 0:
        return 0, []
    return (H - y0) * xs.size, [int(y) * W + int(x) for y, x in zip(rng.integers(y0, H, 16), rng.choice(xs, 16))]


def _delta(rng):
    """A luma delta inside the window (g in [-32, 31], r-g and b-g in
    [-16, 15]), extremes one time in four, never all zero."""
    while True:
        if rng.random() < 0.25:
            g, er, eb = int(rng.choice([-32, 31])), int(rng.choice([-16, 15])), int(rng.choice([-16, 15]))
        else:
            g, er, eb = int(rng.integers(-32, 32)), int(rng.integers(-16, 16)), int(rng.integers(-16, 16))
        if g or er or eb:
            return g + er, g, g + eb


def _in_window(cur, ref):
    g = (cur[1] - ref[1]) & 255
    r = (cur[0] - ref[0] - g) & 255
    b = (cur[2] - ref[2] - g) & 255
    return (g >= 224 or g < 32) and (r >= 240 or r < 16) and (b >= 240 or b < 16)


def _takes(rows, p, W):
    """The kind the encoder gives pixel p of rows (a list of [r, g, b, ...]
    per pixel), from the pixels before it (code.rs:191-339: the first match of
    back references 0..4, small diff, luma2, luma references 0..10), or None
    (rgb, small diff, luma2, a run member).  Only a hint for the planting:
    the oracle's trace decides what counts."""
    cur = rows[p]
    if p == 0 or cur[:3] == rows[p - 1][:3]:
        return None
    for k, off in enumerate(BACK_OFF(W)):
        if 0 < off <= p and cur[:3] == rows[p - off][:3]:
            return ("B", k)
    left = rows[p - 1]
    pred = [(rows[p - W][c] + left[c]) // 2 for c in range(3)] if p >= W else left
    if all(-3 <= cur[c] - pred[c] <= 3 for c in range(3)) or (p >= W and _in_window(cur, pred)):
        return None
    for k, off in enumerate(LUMA_OFF(W)):
        if 0 < off <= p and _in_window(cur, rows[p - off]):
            return ("L", k)
    return None


def planted_frame(W, H, C, seed, cells):
    """Pixels (uint8, W*H*C) of random colours in which each cell is planted up
    to REPEATS times, and one pixel in SPRINKLE takes a random kind.  Cells with
    the fewest possible positions choose first.  The plantings apply in pixel
    order, so a planted pixel's reference already has its final value (a
    pixel's coding depends on earlier pixels only); a luma delta that an
    earlier match would shadow is drawn again a few times, and a planting that
    stays shadowed moves to a later position of its cell."""
    rng = np.random.default_rng(seed)
    N = W * H
    px = rng.integers(0, 256, (N, C), dtype=np.uint8)
    starts = sorted({c[2] for c in cells if c[1] == "d"})

    def free(p, kind, cls):
        """May a cell of this kind and class plant at p?  A back reference
        makes two pixels equal, which shadows what is planted next to it
        whatever the delta: none beside the cells that have one position only
        (class c: the first 3W + 4 pixels; class d: a block's first pixels)."""
        if p in plan or not 0 < offset(kind, W) <= p < N:
            return False
        if kind[0] == "B" and cls not in ("c", "d") and p < 3 * W + 4:
            return False
        return not (kind[0] == "B" and cls != "d" and any(B - 3 <= p < B + 3 for B in starts))

    plan = {}   # position -> (kind, the cell's other candidate positions)
    cand = sorted((_candidates(cell, W, H, rng) + cell[:2] for cell in cells), key=lambda t: t[0])
    for rep in range(REPEATS):
        for n, positions, kind, cls in cand:
            if rep and n == 1:
                continue
            p = next((p for p in positions if free(p, kind, cls)), None)
            if p is not None:
                plan[p] = (kind, cls, positions)
    for p in rng.integers(0, N, N // SPRINKLE):
        kind = KINDS[int(rng.integers(len(KINDS)))]
        if free(int(p), kind, ""):
            plan[int(p)] = (kind, "", ())
    get = _Rows(px)
    todo = sorted(plan)
    heapq.heapify(todo)
    while todo:
        p = heapq.heappop(todo)
        kind, cls, positions = plan[p]
        ref = get[p - offset(kind, W)]
        for _ in range(8):
            d = (0, 0, 0) if kind[0] == "B" else _delta(rng)
            get.set(p, [(ref[c] + d[c]) & 255 for c in range(3)])
            took = _takes(get, p, W)
            if took == kind or kind[0] == "B":
                break
        if took != kind:   # shadowed: the cell tries a later position of its own
            q = next((q for q in positions if q > p and free(q, kind, cls)), None)
            if q is not None:
                plan[q] = plan[p]
                heapq.heappush(todo, q)
    planted_frame.plantings = len(plan)   # the pixels the Python loops touched (tests bound it)
    return px.reshape(-1)


class _Rows:
    """px[p] as a list of python ints, read through to the array and cached."""

    def __init__(self, px):
        self.px, self.cache = px, {}

    def __getitem__(self, p):
        v = self.cache.get(p)
        if v is None:
            v = self.cache[p] = self.px[p, :3].tolist()
        return v

    def set(self, p, rgb):
        self.cache[p] = rgb
        self.px[p, :3] = rgb


def coverage(trace, W, cells):
    """cell -> the number of pixels of its class that the trace shows taking its kind."""
    trace = np.asarray(trace)
    pos = {kind: np.nonzero(trace == CODE(kind))[0] for kind in KINDS}
    hits = {}
    for cell in cells:
        kind, cls, arg = cell
        p = pos[kind]
        if cls in ("a", "g"):
            n = np.count_nonzero(p % W == arg)
        elif cls == "b":
            n = np.count_nonzero(p % TILE == arg)
        elif cls == "c":
            n = np.count_nonzero(p == arg)
        elif cls == "d":
            n = np.count_nonzero((p >= max(arg, offset(kind, W))) & (p < arg + offset(kind, W)))
        else:
            n = np.count_nonzero(p % W % (2048 if cls == "e" else 16) == arg)
        hits[cell] = int(n)
    return hits


# ---------------------------------------------------------------------------
# The shapes of tests/test_ref_offsets.py.  H is the smallest (in steps of 4 from
# the rows the three-row references need) at which the seeds below fill every
# cell of all three variants; tests/test_planted_refs_cpu.py asserts that they do.
# ---------------------------------------------------------------------------
def block_starts(W, H):
    return list(range(BLOCK, W * H, BLOCK))


# (W, H, C) -> what its table adds to classes a, b, c and the block starts
ENC_SHAPES = {
    (332, 150, 4): {}, (334, 150, 4): {}, (335, 150, 4): {},
    (333, 150, 4): {"bands": 3}, (333, 150, 3): {"bands": 3},
    (5000, 24, 4): {}, (5000, 24, 3): {},
    (5120, 32, 4): {"strip": True},
    (10300, 24, 4): {}, (10300, 24, 3): {},
}
TINY_SHAPES = [(w, 40, c) for w in range(1, 8) for c in (3, 4)]
# (W, H, C) -> the wave and strip edges of every route the shape goes through
DEC_SHAPES = {
    (37, 64, 3): [], (61, 64, 3): [],
    (67, 64, 3): strip_edges(67, 2),
    (515, 64, 3): wave_edges(515, 8),
    (1026, 64, 3): wave_edges(1026) + strip_edges(1026, 2) + strip_edges(1026, 3),
    (1026, 64, 4): wave_edges(1026) + strip_edges(1026, 2) + strip_edges(1026, 3),
    # dec_rows_wide and the default three strips of dec_rows_split: nine waves, ten edges
    (8194, 40, 3): wave_edges(8194) + strip_edges(8194, 3),
}


def table(shape, variant):
    W, H, C = shape
    if shape in DEC_SHAPES:
        return cell_table(W, H, variant, starts=block_starts(W, H), decoder=True, edges=sorted(DEC_SHAPES[shape]))
    o = ENC_SHAPES[shape]
    starts = sorted(set(block_starts(W, H) + (band_starts(W, H, o["bands"]) if "bands" in o else [])))
    return cell_table(W, H, variant, starts=starts, strip=o.get("strip", False))


# seeds of variants 0..2 (the first ones tried at which every cell of the table is hit and,
# for the decoder shapes, the oracle's tolerant decode returns the frame)
SEEDS = {
    (332, 150, 4): (1, 101, 201), (334, 150, 4): (1, 101, 201), (335, 150, 4): (2, 101, 201),
    (333, 150, 4): (1, 101, 201), (333, 150, 3): (1, 101, 201),
    (5000, 24, 4): (8, 103, 203), (5000, 24, 3): (3, 104, 208), (5120, 32, 4): (5, 106, 206),
    (10300, 24, 4): (2, 104, 205), (10300, 24, 3): (6, 101, 201),
    (37, 64, 3): (1, 101, 201), (61, 64, 3): (3, 101, 201), (67, 64, 3): (1, 101, 201),
    (515, 64, 3): (1, 101, 201), (1026, 64, 3): (1, 101, 201), (1026, 64, 4): (1, 101, 201),
    (8194, 40, 3): (2, 103, 201),
}


@functools.lru_cache(maxsize=None)
def frame(shape, variant):
    """(pixels, the oracle's stream, its trace, the table) of one of a shape's
    three frames, made once.  The tiny shapes have no table: their offsets
    coincide or wrap, and the trace says which reference wins."""
    from conftest import oracle_mod
    O = oracle_mod()
    W, H, C = shape
    if shape in TINY_SHAPES:
        cells = [c for c in cell_table(W, H, variant) if c[1] == "a" and c[2] >= 0]
        seed = 7 * W + C + variant
    else:
        cells, seed = table(shape, variant), SEEDS[shape][variant]
    px = planted_frame(W, H, C, seed, cells)
    px.setflags(write=False)
    stream, trace = O.encode_trace(px, W, H, C)
    return px, stream, trace, (() if shape in TINY_SHAPES else tuple(cells))
