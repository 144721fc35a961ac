"""The barrier row kernels' body on the CPU, under AddressSanitizer and
UBSan: tools/rows_host_check.cpp compiles csrc/nice_rows_body.hpp -- the text
dec_rows, dec_rows8 and dec_rows_wide compile on the device -- with g++ through
the HIP names of tools/hip_host_shim, runs one block as host threads with every
buffer (LDS, the global ring, records, output) at exactly the planner's size,
and compares every output byte with a sequential reference that uses no ring.
A stand-alone program: nothing is loaded into Python.

Each case is the smallest that can still go wrong: 12 rows (three turns of the
four-row ring), three and four output channels in turn over seven seeds, which
are what the program's coverage condition needs (every record class at every
watched column in every ring slot, and at its first valid pixels; see the
program's header).  The widths: the last segment of 16, 2, 3, 2 and 16 pixels
in one and two waves (dec_rows), 8-pixel segments (dec_rows8), and the
narrowest widths the planner sends to dec_rows_wide, W % 16 of 1, 2, 0 and 3.

What it found in the text before this test existed (all in the 16-pixel
table-form pre-pass): idle lanes reading past the ring (any width whose
segments do not fill the last wave), lane 0's table index going negative and
wrapping as unsigned (harmless in LDS, 16 GiB off in the global ring), and
dec_rows_wide never writing row -1's right halo (pixels 3W-3 .. 3W-1).

Measured on 8 cores: the whole file 46 s (the compile, charged to the first
case, 8 s; dec_rows and dec_rows8 cases under 1 s each; each dec_rows_wide
case, 576 threads, about 8 s)."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

import plan_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 12
SEEDS = range(1, 8)   # seven consecutive seeds take every class through every watched cell
# kernel -> (the program's name for it, the plan options that force it, widths)
KERNELS = {
    "dec_rows": ("rows", {"flow": 0, "split": 0}, (64, 66, 67, 1026, 1600)),
    "dec_rows8": ("rows8", {"seg": 8, "split": 0}, (515,)),
    "dec_rows_wide": ("wide", {"split": 0}, (8193, 8194, 8208, 8211)),
}
CASES = [(k, w) for k, (_, _, widths) in KERNELS.items() for w in widths]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@functools.lru_cache(maxsize=None)
def _exe():
    d = tempfile.mkdtemp(prefix="rows_host_check_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    out = os.path.join(d, "rows_host_check")
    # the sanitizers' runtimes linked statically: the program then runs whatever else the
    # environment loads first (a dynamic ASan runtime refuses to start unless it is the first library)
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-pthread",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "tools", "hip_host_shim"), "-I", plan_driver.CSRC,
                           "-o", out, os.path.join(ROOT, "tools", "rows_host_check.cpp")])
    return out


def _run(args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    return subprocess.run([_exe()] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=env)


@pytest.mark.parametrize("kernel,W", CASES, ids=[f"{k}-{w}" for k, w in CASES])
def test_rows_body_on_host(kernel, W):
    name, options, _ = KERNELS[kernel]
    want = plan_driver.plan(W, H, 1, 256, **options)
    assert want["route"] == kernel   # the width goes where the case says
    if kernel == "dec_rows":
        assert (W % 16, want["threads"]) == {64: (0, 64), 66: (2, 64), 67: (3, 64), 1026: (2, 128), 1600: (0, 128)}[W]
    if kernel == "dec_rows_wide":
        assert want["threads"] == 576 and plan_driver.plan(8192, H, 1, 256, **options)["route"] != kernel
    out = _run([name, W, H, "3,4", *SEEDS])
    report = out.stdout + out.stderr
    assert out.returncode == 0, report
    assert "runtime error" not in report and "Sanitizer" not in report, report
    line = out.stdout.strip().splitlines()[-1].split()
    assert line[-1] == "OK" and f"kernel={name}" in line and f"W={W}" in line and f"threads={want['threads']}" in line
    assert {"wrong_pixels=0", "status=0", "empty_cells=0", f"seeds={len(SEEDS)}"} <= set(line), line


def test_coverage_condition_is_checked():
    """One seed cannot fill the cells: the program says so and fails, with the pixels right."""
    out = _run(["rows", 66, H, 3, 1])
    assert out.returncode == 1, out.stdout + out.stderr
    line = out.stdout.strip().splitlines()[-1].split()
    assert line[-1] == "FAIL" and "wrong_pixels=0" in line and "empty_cells=0" not in line
    assert "no record: class" in out.stderr
