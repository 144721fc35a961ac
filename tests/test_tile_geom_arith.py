"""The tile kernels' geometry (csrc/nice_tile_geom.hpp, the header that
nice_tiles.hip, nice_sets.hip and the tensor merges compile) against brute
force: the cut of a tile to its band, window and image equals the per-pixel
definition, the split of a wave between a row's groups and the rows below is
the least power of two that holds the groups, and the vector mode of a base
and its pitches equals trying every width: tools/tile_geom_check.cpp, built by
tools/Makefile with plain g++ (CPU only)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_tile_geom_equal(tmp_path):
    exe = str(tmp_path / "tile_geom_check")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools"), exe, "OUT=" + str(tmp_path) + os.sep])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tile_cut 0, row_share 0, vector_mode 0, byte_mode 0 mismatches" in out.stdout
