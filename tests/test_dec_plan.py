"""The decoder's launch planner (plan_decode, csrc/nice_dec_plan.hpp) on the
CPU: tools/dec_plan_check.cpp, compiled here with g++ against the two HIP-free
headers the library itself plans with."""
import functools
import re
import shutil
import subprocess

import pytest

import plan_driver

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@functools.lru_cache(maxsize=None)
def _sweep():
    """Every W in 1..40000 x n_frames in {1, 2, 64, 128, 129, 256, 257, 512} at
    256 CUs, no options: (plans checked, [(w, n_frames, mask)], plans refused,
    narrowest refused W).  mask: 1 LDS, 2 block size, 4 split strips, 8 flow
    groups; << 8 for the fallback launch."""
    out = subprocess.run([plan_driver.exe(), "sweep"], capture_output=True, text=True, timeout=300).stdout
    total = re.search(r"checked (\d+) plans, (\d+) violations, (\d+) refused from w=(\d+)", out)
    bad = [(int(w), int(n), int(m, 16)) for w, n, m in re.findall(r"violation w=(\d+) n_frames=(\d+) mask=(0x[0-9a-f]+)", out)]
    assert total and int(total.group(2)) == len(bad), out[-2000:]
    return int(total.group(1)), bad, int(total.group(3)), int(total.group(4))


def test_plan_sweep_blocks_strips_groups():
    """(a) without the LDS bound: the block size is a positive multiple of 64
    within the kernel's launch bound, a split plan has every strip between 2
    and 256 segments, a flow plan has 1 <= k <= 4, k * waves_per_row <= 8 and
    k + 3 ring rows -- for the route and the fallback of every plan."""
    n, bad, refused, refused_from = _sweep()
    assert n == 40000 * 8
    assert [b for b in bad if b[2] & ~0x0101] == []
    # refused (no kernel, the call returns NICE_E_ARG) only where dec_reconstruct, the one kernel for rows
    # of more than 16384 pixels when the strips give up, cannot hold a row's records (4 B per pixel) in LDS
    assert (refused_from, refused) == (39345, (40000 - 39345 + 1) * 8)


def test_plan_sweep_lds():
    """(a), the LDS bound: dynamic LDS plus 1 KB of static LDS is at most 160 KB
    for the route and the fallback of every plan."""
    _, bad, _, _ = _sweep()
    lds = [b for b in bad if b[2] & 0x0101]
    assert lds == [], f"{len(lds)} plans over the LDS bound, e.g. {lds[:3]} ... {lds[-3:]}"


# cus = 256, no options set
TABLE = [
    (32, 1, dict(route="dec_reconstruct", fallback="none")),
    (1920, 1, dict(route="dec_rows_flow", flow_k=2, flow_ring=8, threads=256, lds=68816,
                   fallback="dec_rows", fb_threads=128, fb_lds=36640)),
    (1920, 512, dict(route="dec_rows_flow", flow_k=1, flow_ring=4, threads=128, lds=35792)),
    (3840, 1, dict(route="dec_rows_flow", flow_k=2, flow_ring=8, threads=512, lds=134096)),
    (5000, 1, dict(route="dec_rows_flow", flow_k=1, flow_ring=4, threads=320, lds=88144, fallback="dec_rows")),
    (8192, 1, dict(route="dec_rows_flow", flow_k=1, flow_ring=4, threads=512, lds=142416,
                   fallback="dec_rows", fb_lds=154016)),
    (8208, 1, dict(route="dec_rows_split", strips=3, lds=83968, fallback="dec_rows_wide", fb_threads=576)),
    (8208, 64, dict(route="dec_rows_wide", fallback="none")),
    (20000, 4, dict(route="dec_rows_split", strips=5, split_frames=4, fallback="dec_reconstruct")),
]


@pytest.mark.parametrize("w,n_frames,want", TABLE, ids=[f"{w}x{n}" for w, n, _ in TABLE])
def test_plan_table(w, n_frames, want):
    """(b) Plans derived by hand from the planner's rules."""
    got = plan_driver.plan(w, 8, n_frames, 256)
    assert {k: got[k] for k in want} == want
