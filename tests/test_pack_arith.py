"""The pack kernels' arithmetic (csrc/nice_pack.hpp, the header the kernels of
nice_pack.hip compile) against brute force: the run digits by the table route
equal the plain base-8 digits of run - 1 (code.rs:391-406), the run after a
pixel from a flag word equals a scan, a span of bits lands in the words a count
gives, and the wrapped write's window equals the reference writer's bytes
(bitwriter.rs:55-73): tools/pack_arith_check.cpp, which includes that header by
its path and is compiled here with g++ (CPU only)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_pack_arith_equal(tmp_path):
    exe = str(tmp_path / "pack_arith_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tools", "pack_arith_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "digits 0, run 0, span 0, wrapped 0 mismatches" in out.stdout
