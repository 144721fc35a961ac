"""The encoder's launch planner (plan_encode, csrc/nice_enc_plan.hpp) on the
CPU: tools/enc_plan_check.cpp, compiled here with g++ against the HIP-free
headers the library itself plans with."""
import re
import shutil
import subprocess

import pytest

import plan_driver

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_plan_sweep():
    """Every W in 1..20000 x channels {3, 4} x heights {1, 8, 2160} x {unaligned,
    4-byte, 16-byte aligned} x (batches of 1, 2, 64, 512 frames + four bands of
    one image) at 256 CUs: the kind is legal for the shape, the classify blocks
    cover the work with none empty, ring kernels get 16..16384 tiles per block,
    strip blocks 1..rows rows, every grid is launchable with the kernel's own
    block size, enc_rundigits runs exactly for frames of the staged kernels, and
    enc_pack stays within its persistent grid."""
    r = subprocess.run([plan_driver.enc_exe(), "sweep"], capture_output=True, text=True, timeout=300)
    total = re.search(r"checked (\d+) plans, (\d+) violations", r.stdout)
    assert total, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(total.group(1)) == 20000 * 2 * 3 * 3 * (4 + 4)
    assert (int(total.group(2)), r.returncode) == (0, 0), r.stdout[:4000]


# (w, h, channels, n_frames) -> kind: tests/test_classify_routes.py's frames, the narrow and the
# misaligned shapes of its three added routes, and the rule's edges
KINDS = [((7680, 64, 4, 1), "ring2"), ((6000, 32, 3, 1), "ring2"), ((10239, 9, 4, 1), "ring2"),
         ((10239, 11, 3, 1), "ring2"), ((4777, 20, 4, 1), "ring"), ((4778, 20, 3, 1), "ring2"),
         ((4095, 20, 4, 1), "slide"), ((4095, 20, 3, 1), "ring"), ((1000, 30, 4, 1), "slide"),
         ((8192, 12, 4, 1), "strip"), ((10240, 5, 3, 1), "twin"), ((11000, 5, 4, 1), "twin"),
         ((10241, 9, 3, 1), "twin"), ((12000, 7, 4, 1), "twin"), ((20000, 5, 3, 1), "twin"),
         ((7680, 256, 4, 2), "ring2"), ((2, 5, 4, 1), "tiny"), ((3, 5, 4, 1), "slide"), ((4096, 8, 4, 1), "ring"),
         ((5120, 8, 4, 1), "strip"), ((5120, 8, 3, 1), "ring2"), ((10240, 8, 4, 1), "strip")]


@pytest.mark.parametrize("shape,kind", KINDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_plan_kinds(shape, kind):
    w, h, c, n = shape
    p = plan_driver.enc_plan(w, h, c, n, 256)
    assert (p["kind"], plan_driver.CLS_KINDS[p["kind_id"]]) == (kind, kind)


def test_plan_kinds_alignment_and_options():
    """Memory that is not 4-byte aligned takes the window kernel (a narrow frame
    the tiny one), 4-byte but not 16-byte aligned RGBA the pair kernel; the A/B
    options step down slide -> pair -> ring -> window."""
    P = plan_driver.enc_plan
    assert P(5, 5, 3, 2, 256, al4=0, al16=0)["kernel"] == "enc_classify"
    assert P(2, 5, 3, 2, 256, al4=0, al16=0)["kernel"] == "enc_classify_tiny"
    assert P(5, 5, 4, 2, 256, al16=0)["kernel"] == "enc_classify_pair_m"
    assert P(5, 5, 4, 2, 256)["kernel"] == "enc_classify_slide1"
    assert P(1920, 8, 4, 1, 256, no_slide=1)["kernel"] == "enc_classify_pair_m"
    assert P(1920, 8, 4, 1, 256, no_pair=1)["kernel"] == "enc_classify_ring_m"
    assert P(1920, 8, 4, 1, 256, no_ring=1)["kernel"] == "enc_classify"


def _band_tiles(w, h, R):
    """sharded.encode_bands' split of the T tiles over R ranks."""
    T = (w * h + 1023) // 1024
    return [(r * T // R, (r + 1) * T // R) for r in range(R)]


# tests/test_classify_routes.py's bands: never the slide kernel, no coded flags out, no enc_rundigits
BANDS = [((1920, 1080, 4, 4), "pair", "enc_classify_pair"), ((1000, 700, 3, 3), "ring", "enc_classify_ring3"),
         ((7680, 300, 4, 3), "ring2", "enc_classify_ring2"), ((8192, 200, 4, 2), "strip", "enc_classify_strip"),
         ((11000, 60, 4, 3), "twin", "enc_classify_twin"), ((10300, 50, 3, 2), "twin", "enc_classify_twin3")]


@pytest.mark.parametrize("shape,kind,kernel", BANDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_plan_bands(shape, kind, kernel):
    w, h, c, R = shape
    for lo, hi in _band_tiles(w, h, R):
        p = plan_driver.enc_plan(w, h, c, 1, 256, band=(lo, hi))
        assert (p["kind"], p["kernel"], p["flags_out"], p["rd_x"], p["cmask_std"]) == (kind, kernel, 0, 0, 0)
        assert (p["tile_lo"], p["tile_hi"]) == (lo, hi)


def test_plan_band_numbers():
    """The second of two bands of 8192 x 200 RGBA (tiles 800..1600, 8 per row:
    rows 100..199): 4 strips x 100 rows over 768 wanted blocks -> 16 rows per
    block, 4 x 7 blocks; 200 pack groups -> one block of enc_edges, sized from
    the groups (frames size it from the tiles)."""
    p = plan_driver.enc_plan(8192, 200, 4, 1, 256, band=(800, 1600))
    want = dict(kernel="enc_classify_strip", tiles_per_block=16, cls_x=28, cls_threads=512, rd_x=0, groups=1, gr_x=0,
                tr_x=1, tr_y=1, long_x=800, pack_x=800, pack_slots=1, over_x=64, edges_x=1, edges_y=1, tail_x=1)
    assert {k: p[k] for k in want} == want
    # the same tiles as a frame: the edges grid comes from the 1600 tiles
    f = plan_driver.enc_plan(8192, 200, 4, 1, 256)
    assert (f["edges_x"], f["edges_y"], f["pack_x"], f["long_x"]) == (7, 1, 1024, 1600)


# full plans at 256 CUs, 16-byte aligned frames, worked out by hand from the rules
TABLE = [
    # 8100 tiles per frame; 2 x 256 ring blocks; run digits max(64, 2048 / 512) columns; 1024 = 4 x 256 pack
    # blocks over 64 slots of 8 frames; edges ceil(8100 / 256) = 32 columns
    ((3840, 2160, 4, 512), dict(kind="slide", kernel="enc_classify_slide0", cls_x=512, cls_threads=512,
                                tiles_per_block=8100, rd_x=64, rd_y=512, rd_threads=256, il=1, cmask_std=1, groups=1,
                                gr_x=0, tr_x=1, tr_y=512, ts_x=1, ts_y=512, tables_x=5120, header_x=512,
                                packtab_x=512, long_x=2048, pack_x=1024, pack_slots=64, over_x=64, edges_x=32,
                                edges_y=512, tail_x=8)),
    # 30 tiles: the ring kernels' 16 tiles per block at least
    ((1000, 30, 4, 1), dict(kind="slide", kernel="enc_classify_slide0", cls_x=2, tiles_per_block=16, rd_x=4, rd_y=1,
                            il=1, long_x=30, pack_x=30, pack_slots=1, edges_x=1, edges_y=1, tail_x=1)),
    # 4 strips of 2048 columns x 12 rows: fewer than 16 rows, one block per strip
    ((8192, 12, 4, 1), dict(kind="strip", kernel="enc_classify_strip_m", cls_x=4, tiles_per_block=12, rd_x=12, il=0,
                            cmask_std=1)),
    # 98 tiles over 512 twin blocks: one each
    ((20000, 5, 3, 1), dict(kind="twin", kernel="enc_classify_twin3_m", cls_x=98, tiles_per_block=1, rd_x=13, il=0)),
    # window kernel (unaligned): 2048 blocks of 256 threads, no run-digit pass
    ((1920, 1080, 3, 2), dict(kind="window", kernel="enc_classify", cls_x=2025, cls_threads=256, tiles_per_block=2,
                              rd_x=0, cmask_std=0, flags_out=0), dict(al4=0, al16=0)),
    # 8 x 20000 x 2160 RGB: 42188 tiles per frame, 6 scan groups of 8192
    ((20000, 2160, 3, 8), dict(kind="twin", groups=6, gr_x=6, gr_y=8, tr_x=6, tr_y=8, ts_x=6, ts_y=8, edges_x=64,
                               edges_y=8, pack_slots=8, pack_x=1024, long_x=2048)),
]


@pytest.mark.parametrize("case", TABLE, ids=lambda c: "x".join(map(str, c[0])))
def test_plan_table(case):
    (w, h, c, n), want = case[0], case[1]
    got = plan_driver.enc_plan(w, h, c, n, 256, **(case[2] if len(case) > 2 else {}))
    assert {k: got[k] for k in want} == want
