"""The slot planner of the tiled and set decodes (csrc/nice_slot_plan.hpp) on
the CPU: tools/slot_plan_check.cpp, compiled here with g++ against the HIP-free
header the library itself plans with."""
import re
import shutil
import subprocess

import pytest

import plan_driver

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_sweep():
    """Both planners against the brute-force slot list: the slot count of
    nice_set_select, order and positions, every position coded, raw / sourced
    or refused and exactly one of those, tile indices inside their image, the
    cut tiles covering every window pixel once, and the packer's columns
    disjoint, naturally aligned, the tail 16-byte aligned.

    One-image sets: the 91840 cases of one axis (extent 1..40, tile 2..9, every
    window interval) for the columns, each joined with 8 of the same 91840
    cases for the rows.  Every image and tile size and every window of either
    axis occurs, 8 times; the full product of the two axes, 91840^2 = 8.4e9
    sets, is out of a test's reach, and the planner's two axes meet only in the
    raster order and the tile index, which every joined case exercises.  Then
    20000 three-image sets of one to four windows from a fixed seed.  Two plans
    (colour, alpha) per set."""
    run = subprocess.run([plan_driver.slot_exe(), "sweep"], capture_output=True, text=True, timeout=300)
    total = re.search(r"checked (\d+) plans, (\d+) violations", run.stdout)
    assert total, run.stdout[-2000:] + run.stderr[-2000:]
    assert (int(total.group(1)), int(total.group(2))) == (2 * (8 * 91840 + 20000), 0), run.stdout[-2000:]
    assert run.returncode == 0


def test_rules():
    """The literal table: every branch of the colour and the alpha rule list
    with its status or class, the boundaries (off == bytes with len == 0,
    len == bytes - off) among them, and the tiled plan equal to the one-image,
    one-window set's, column for column."""
    run = subprocess.run([plan_driver.slot_exe(), "rules"], capture_output=True, text=True, timeout=60)
    total = re.search(r"checked (\d+) entries, (\d+) failures", run.stdout)
    assert total, run.stdout[-2000:] + run.stderr[-2000:]
    assert (int(total.group(1)), int(total.group(2))) == (21, 0), run.stdout[-2000:]
    assert run.returncode == 0
