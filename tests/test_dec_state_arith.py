"""The decoder's packed state words and pixel arithmetic (csrc/nice_dec_state.hpp,
the header the kernels of nice_decode.hip compile): the one pixel_count equals
the 64-bit formula (count and next dk) for every prefix x dk in 0..64, and the
slice entry, `last` and checkpoint words round-trip at their field limits:
tools/dec_state_check.cpp, which includes that header by its path and is
compiled here with g++ (CPU only)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_dec_state_arith_equal(tmp_path):
    exe = str(tmp_path / "dec_state_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tools", "dec_state_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "count 0, word 0 mismatches" in out.stdout
