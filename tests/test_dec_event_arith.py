"""The decoder's event-word arithmetic (csrc/nice_dec_event.hpp, the header the
kernels of nice_decode.hip compile): dec_place's record from the event word
dec_sync keeps, place_record(ev_pack(prefix, symbols), q), equals dec_emit's
record from the symbols, make_record -- record and bad flag, every prefix,
every symbol tuple of the streams' alphabets (RGB: all 2^24), every reference
id 0..15, q in 0 .. 3W + 5 and one large q, W in {1, 2, 3, 4, 7, 64}, with the
position checks and (where the hoisting rule selects it) without:
tools/dec_event_check.cpp, which includes that header by its path and is
compiled here with g++ (CPU only)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_dec_event_arith_equal(tmp_path):
    exe = str(tmp_path / "dec_event_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tools", "dec_event_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "word 0, record 0, flag 0 mismatches" in out.stdout
