"""CPU-side checks of the product boundary: the C-ABI library builds, loads and
exports every entry point include/nice.h declares (no compute calls here)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT, nice_pkg


def _declared():
    hdr = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("nice.h", "nice_test.h"))
    return sorted(set(re.findall(r"\b(nice_[a-z_0-9]+)\s*\(", hdr)))


def test_header_declares_boundary():
    names = _declared()
    for n in ("nice_encode", "nice_decode", "nice_encode_bound", "nice_peek_header",
              "nice_encode_batch_dev", "nice_decode_batch_dev", "nice_ctx_create"):
        assert n in names


def test_library_exports_every_declared_symbol():
    pkg = nice_pkg()
    # torch first, as lib() does: loaded before it, the library binds to the system's HIP
    # runtime instead of the one torch brings, and a later GPU test in this process finds
    # no device (two runtimes in one process)
    pkg.lib()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for n in _declared():
        assert hasattr(L, n), n
    assert set(pkg.EXPORTS) <= set(_declared())


_WIDTH = {"uint8_t": 1, "uint32_t": 4, "int": 4, "int32_t": 4, "float": 4, "uint64_t": 8, "size_t": 8, "int64_t": 8}


def _c_class(text):
    """A C parameter or return type as "void", "ptr" or its width in bytes."""
    if "*" in text:
        return "ptr"
    words = [w for w in text.split() if w != "const"]
    if words[0] == "void":
        return "void"
    return _WIDTH[words[0]]


def _prototypes():
    """{name: (return class, [parameter classes])} of every nice_* prototype in the two headers."""
    hdr = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("nice.h", "nice_test.h"))
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    hdr = re.sub(r"^\s*#[^\n]*", " ", hdr, flags=re.M)
    protos = {}
    for chunk in hdr.split(";"):
        chunk = re.split(r"[{}]", chunk)[-1].strip()
        m = re.fullmatch(r"(.*?)\b(nice_[a-z_0-9]+)\s*\((.*)\)", chunk, flags=re.S)
        if not m or chunk.startswith("typedef"):
            continue
        params = [p.strip() for p in m.group(3).split(",")]
        protos[m.group(2)] = (_c_class(m.group(1)), [] if params == ["void"] else [_c_class(p) for p in params])
    return protos


def _ctypes_class(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "ptr"
    return ctypes.sizeof(t)


def test_ctypes_signatures_match_header(monkeypatch):
    """Every function the package annotates (``argtypes``, or a ``restype``
    other than ctypes' default int) agrees with its prototype in include/nice.h
    or include/nice_test.h: the parameter count, and position by position, as
    for the return type, pointer against pointer or the byte width of the
    scalar.  Beside ``lib()``'s block this covers what png.py and sharded.py
    annotate: ``png._unfilter`` and ``sharded.tile_pixels`` run on the host;
    ``sharded.HipBands`` creates a device context before it annotates, so here
    it is given a stand-in for ``_ctx`` and only its annotations are used."""
    import importlib
    pkg = nice_pkg()
    L = pkg.lib()
    protos = _prototypes()
    assert set(pkg.EXPORTS) <= set(protos) and set(protos) == set(_declared())
    importlib.import_module(pkg.__name__ + ".png")._unfilter(b"\0\x07", 1, 1, 1)
    sharded = importlib.import_module(pkg.__name__ + ".sharded")
    assert sharded.tile_pixels() > 0
    monkeypatch.setattr(pkg, "_ctx", lambda device: None)
    sharded.HipBands(0)
    checked = 0
    for name, (ret, params) in sorted(protos.items()):
        fn = getattr(L, name)
        if fn.argtypes is None and fn.restype is ctypes.c_int:
            continue
        checked += 1
        assert _ctypes_class(fn.restype) == ret, f"{name}: restype {fn.restype} against {ret}"
        if fn.argtypes is not None:
            got = [_ctypes_class(t) for t in fn.argtypes]
            assert got == params, f"{name}: argtypes {got} against {params}"
    assert checked >= 50 and L.nice_ctx_destroy.restype is None and L.nice_pipe_destroy.restype is None
    for name in ("nice_decode_set_tensor_dev", "nice_png_unfilter", "nice_tile_pixels", "nice_band_assemble"):
        fn = getattr(L, name)
        assert fn.argtypes is not None or fn.restype is not ctypes.c_int, name


def test_encode_bound_and_header_parse():
    pkg = nice_pkg()
    L = pkg.lib()
    assert L.nice_encode_bound(3840, 2160) >= 3840 * 2160 * 4
    hdr = b"nice" + (3840).to_bytes(4, "big") + (2160).to_bytes(4, "big") + bytes([3])
    w, h, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint8()
    buf = ctypes.create_string_buffer(hdr, len(hdr))
    assert L.nice_peek_header(buf, len(hdr), ctypes.byref(w), ctypes.byref(h), ctypes.byref(c)) == 0
    assert (w.value, h.value, c.value) == (3840, 2160, 3)


def test_library_reads_no_environment():
    """Internal routes are forced through nice_test_set_option (include/nice_test.h),
    never by environment variables: the library names none and imports no getenv."""
    pkg = nice_pkg()
    blob = open(pkg.LIB_PATH, "rb").read()
    assert b"NICE_DEC_" not in blob and b"NICE_ENC_" not in blob
    assert b"getenv" not in blob
    for f in os.listdir(os.path.join(ROOT, "fast-losless-image-compression-format_amd", "csrc")):
        text = open(os.path.join(ROOT, "fast-losless-image-compression-format_amd", "csrc", f)).read()
        assert "getenv" not in text, f


def test_no_oracle_in_product():
    """The product library never links or loads the oracle."""
    pkg = nice_pkg()
    blob = open(pkg.LIB_PATH, "rb").read()
    assert b"nice_oracle" not in blob
    src_dir = os.path.join(ROOT, "fast-losless-image-compression-format_amd")
    for dirpath, _, files in os.walk(src_dir):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp", ".cpp", "Makefile")):
                text = open(os.path.join(dirpath, f)).read()
                assert "liboracle" not in text and "nice_oracle" not in text, f
                assert "from oracle" not in text and "import oracle" not in text, f


def test_cpp_mirror_compiles(tmp_path):
    """include/nice.hpp (C++ mirror of code::encode/decode) compiles against nice.h
    and links libnice_hip.so with plain g++."""
    import subprocess
    subprocess.check_call(["make", "-s", "-B", "-C", os.path.join(ROOT, "examples"), "roundtrip"])
    assert os.path.exists(os.path.join(ROOT, "examples", "roundtrip"))


@pytest.mark.gpu
def test_cpp_mirror_roundtrip(tmp_path, O):
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "roundtrip"])
    path = str(tmp_path / "s.nice")
    out = subprocess.run([os.path.join(ROOT, "examples", "roundtrip"), "1283", "719", path],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok")
    # the example's frame is NICE-SYN-v1 seed 1: its stream is the oracle's
    assert open(path, "rb").read() == O.encode(O.gen_syn_v1(1283, 719, 4, 1), 1283, 719, 4)


def test_checksum64_definition():
    """checksum64 (include/nice.h, nice_pipe_set_checksums) against its
    definition written out word by word, odd lengths zero-padded."""
    pkg = nice_pkg()
    import numpy as np
    rng = np.random.default_rng(5)
    for n in (0, 1, 3, 4, 5, 17, 1001):
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        p = b + bytes(-n % 4)
        A = B = 0
        for i in range(len(p) // 4):
            wv = int.from_bytes(p[4 * i:4 * i + 4], "little")
            A += wv
            B += (i + 1) * wv
        want = (A + 0x9E3779B97F4A7C15 * B) % (1 << 64)
        assert pkg.checksum64(b) == want, n
