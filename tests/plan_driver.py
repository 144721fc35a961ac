"""The planners on the CPU (tools/dec_plan_check.cpp, tools/enc_plan_check.cpp
and tools/slot_plan_check.cpp, built here with g++ once per session) and the
library's reports of what it took (nice_test_last_dec_route,
nice_test_last_classify), for the tests that compare the two."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-losless-image-compression-format_amd", "csrc")

# DecRoute (csrc/nice_dec_plan.hpp)
ROUTE_IDS = {"none": 0, "dec_reconstruct": 1, "dec_rows": 2, "dec_rows8": 3, "dec_rows_wide": 4,
             "dec_rows_flow": 5, "dec_rows_split": 6}
ROUTE_NAMES = {v: k for k, v in ROUTE_IDS.items()}


# ClsKind (csrc/nice_enc_plan.hpp)
CLS_KINDS = ("window", "tiny", "ring", "ring2", "strip", "pair", "twin", "slide")


@functools.lru_cache(maxsize=None)
def _build(name):
    d = tempfile.mkdtemp(prefix=name + "_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    out = os.path.join(d, name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", out,
                           os.path.join(ROOT, "tools", name + ".cpp")])
    return out


def exe():
    return _build("dec_plan_check")


def enc_exe():
    return _build("enc_plan_check")


def slot_exe():
    return _build("slot_plan_check")


def plan(w, h, n_frames, cus, **options):
    """One plan as a dict: route / fallback by kernel name, the numbers as ints.
    options: single_wave, seg, split, flow (unset unless given)."""
    args = [exe(), "plan", str(w), str(h), str(n_frames), str(cus)] + [f"{k}={v}" for k, v in options.items()]
    line = subprocess.run(args, capture_output=True, text=True, check=True, timeout=60).stdout
    kv = dict(f.split("=") for f in line.split())
    return {k: v if k in ("route", "fallback") else int(v) for k, v in kv.items()}


def last_route(nice, ctx=None):
    """(route, fallback) kernel names of the last decode on ctx (None: the
    context behind decode_bytes)."""
    L = nice.lib()
    L.nice_test_last_dec_route.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                                           ctypes.POINTER(ctypes.c_uint32)]
    r, f = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.nice_test_last_dec_route(ctx.ptr if ctx is not None else None, ctypes.byref(r), ctypes.byref(f)) == 0
    return ROUTE_NAMES[r.value], ROUTE_NAMES[f.value]


def enc_plan(w, h, channels, n_frames, cus, band=None, **options):
    """One encode plan as a dict: kind / kernel by name, the numbers as ints.
    band: (tile_lo, tile_hi) of one image.  options: al4, al16 (1 unless
    given), no_ring, no_pair, no_slide (0 unless given)."""
    args = [enc_exe(), "plan", str(w), str(h), str(channels), str(n_frames), str(cus)]
    if band is not None:
        args.append(f"band={band[0]}:{band[1]}")
    args += [f"{k}={int(v)}" for k, v in options.items()]
    line = subprocess.run(args, capture_output=True, text=True, check=True, timeout=60).stdout
    kv = dict(f.split("=") for f in line.split())
    return {k: v if k in ("kind", "kernel") else int(v) for k, v in kv.items()}


def last_classify(nice, ctx):
    """ClsKind of the last encode (or band classify) on ctx."""
    L = nice.lib()
    L.nice_test_last_classify.argtypes = [ctypes.c_void_p]
    L.nice_test_last_classify.restype = ctypes.c_int
    return L.nice_test_last_classify(ctx.ptr)
