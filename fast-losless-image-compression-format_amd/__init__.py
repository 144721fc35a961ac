"""MI355X-native NICE2 codec: host-side mirror of the reference codec API.

The reference (Rust, wouter-rombouts/fast-losless-image-compression-format)
exposes its codec path as

* ``image::Image::new(width, height, channels)``          image.rs:22-43
* ``code::encode(input_bytes, image_header, channels_out, output_writer)``
                                                            code.rs:59-64
* ``code::decode(image_reader, channels_out, output_vec) -> Image``
                                                            code.rs:464-468

This package keeps those names and argument meanings and forwards to the C ABI
in ``libnice_hip.so`` (include/nice.h), whose kernels run on the GPU.  There is
no CPU fallback: if the library or a gfx950 device is missing, every call raises.

Device-resident batches (the benchmark path) go through ``encode_batch`` and
``decode_batch`` which take torch tensors already on the GPU.
"""
from __future__ import annotations

import ctypes
import io
import os
from dataclasses import dataclass

__all__ = [
    "Image", "encode", "decode", "encode_bytes", "decode_bytes", "encode_bound",
    "encode_batch", "decode_batch", "Context", "Pipeline", "NiceError", "lib", "LIB_PATH",
    "packed_bound", "pack_streams", "encode_batch_packed", "decode_batch_packed", "save_packed", "load_packed",
    "TiledImage", "TiledAlpha", "tiled_alpha_bound", "tile_grid", "tile_select", "tiled_bound", "encode_tiled", "decode_tiled", "save_tiled",
    "load_tiled", "DEFAULT_TILE",
    "ImageSet", "set_grid", "set_select", "set_bound", "set_alpha_bound", "encode_set", "decode_set", "save_set",
    "load_set", "DEFAULT_SET_TILE", "decode_set_tensor", "normalize_affine", "decode_set_resized",
    "DEC_STRICT_REFERENCE", "DEC_ALPHA_FILL_FF", "DEC_TOLERANT_HEADER",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
# NICE_LIB_PATH: an alternative build of the same library (tools/ A/B timing)
LIB_PATH = os.environ.get("NICE_LIB_PATH") or os.path.join(_HERE, "libnice_hip.so")

OK, E_ARG, E_HIP, E_NODEV, E_CAPACITY, E_FORMAT, E_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6
_ERRNAMES = {E_ARG: "bad argument", E_HIP: "HIP runtime failure", E_NODEV: "no gfx950 device",
             E_CAPACITY: "output buffer too small",
             E_FORMAT: "malformed stream (the reference decoder would panic)",
             E_UNSUPPORTED: "stream outside the reference decoder's domain"}
DEC_STRICT_REFERENCE = 0x1
DEC_ALPHA_FILL_FF = 0x2
DEC_TOLERANT_HEADER = 0x4   # repair spilled 5-bit max fields (small / flat images)

EXPORTS = [
    "nice_version", "nice_device_count", "nice_encode_bound", "nice_encode", "nice_peek_header",
    "nice_decode", "nice_ctx_create", "nice_ctx_destroy", "nice_ctx_reserve",
    "nice_encode_batch_dev", "nice_decode_batch_dev", "nice_decode_batch_dev_hl",
    "nice_band_classify", "nice_band_runs", "nice_band_tables", "nice_band_words", "nice_band_pack",
    "nice_band_runs_dev", "nice_band_tables_dev", "nice_band_pack_bits",
    "nice_band_assemble", "nice_tile_pixels",
    "nice_pipe_create", "nice_pipe_destroy", "nice_pipe_stream_stride", "nice_pipe_encode",
    "nice_pipe_decode", "nice_pipe_set_checksums",
    "nice_packed_bound", "nice_pack_streams_dev", "nice_encode_batch_packed_dev", "nice_decode_packed_dev",
    "nice_tile_grid", "nice_tiled_bound", "nice_tile_select", "nice_tiles_split_dev", "nice_tiles_merge_dev",
    "nice_encode_tiled_dev", "nice_decode_tiled_dev",
    "nice_tile_alpha_width", "nice_tiled_alpha_bound", "nice_tiles_alpha_range_dev", "nice_encode_tiled_alpha_dev",
    "nice_decode_tiled_alpha_dev",
    "nice_set_grid", "nice_set_bound", "nice_set_select", "nice_set_split_dev", "nice_set_merge_dev",
    "nice_encode_set_dev", "nice_decode_set_dev",
    "nice_set_alpha_bound", "nice_set_alpha_range_dev", "nice_encode_set_alpha_dev", "nice_decode_set_alpha_dev",
    "nice_set_merge_tensor_dev", "nice_decode_set_tensor_dev",
    "nice_set_resize_tensor_dev", "nice_decode_set_resized_dev",
    "nice_set_resize_aa_tensor_dev", "nice_decode_set_resized_aa_dev",
]
TENSOR_F32, TENSOR_F16, TENSOR_BF16 = 0, 1, 2
TENSOR_PLANAR, TENSOR_INTERLEAVED = 0, 1
RESIZE_MAX = 8192
RESIZE_AA_MAX_IN = 65536


class NiceError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        super().__init__(f"{what}: {_ERRNAMES.get(code, 'error')} ({code})")


_lib = None


def lib():
    """Load libnice_hip.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NiceError(E_NODEV, f"{LIB_PATH} missing (run __graft_entry__.build())")
    # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7; load it
    # first so libnice_hip.so binds to the same runtime (same SONAME) and device
    # pointers / streams are shared with torch.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _signatures().items():
        fn = getattr(L, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    _lib = L
    return L


def _signatures():
    """{entry point: (restype, argtypes)} of what this module calls, as
    include/nice.h declares it (tests/test_abi.py holds each against its
    prototype); ``argtypes`` None: no parameters."""
    i, z, u8, u32, u64, p = (ctypes.c_int, ctypes.c_size_t, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64,
                             ctypes.c_void_p)
    pz, pu8, pu32, pp = ctypes.POINTER(z), ctypes.POINTER(u8), ctypes.POINTER(u32), ctypes.POINTER(p)
    return {
        "nice_version": (ctypes.c_char_p, None),
        "nice_encode_bound": (z, [u32, u32]),
        "nice_encode": (i, [p, z, u32, u32, u8, u8, p, z, pz]),
        "nice_peek_header": (i, [p, z, pu32, pu32, pu8]),
        "nice_decode": (i, [p, z, p, z, u32, pz]),
        "nice_ctx_create": (i, [i, pp]),
        "nice_ctx_destroy": (None, [p]),
        "nice_ctx_reserve": (i, [p, u32, u32, u32]),
        "nice_encode_batch_dev": (i, [p, p, p, u64, u32, u32, u32, u8, u8, p, u64, p]),
        "nice_decode_batch_dev": (i, [p, p, p, u64, p, u32, u32, u32, u8, p, u64, u32, p]),
        "nice_decode_batch_dev_hl": (i, [p, p, p, u64, p, p, u32, u32, u32, u8, p, u64, u32, p]),
        "nice_packed_bound": (u64, [u32, u32, u32]),
        "nice_pack_streams_dev": (i, [p, p, p, u64, p, u32, p, u64, p, p]),
        "nice_encode_batch_packed_dev": (i, [p, p, p, u64, u32, u32, u32, u8, u8, p, u64, p, p, p]),
        "nice_decode_packed_dev": (i, [p, p, p, u64, p, p, p, u32, u32, u32, u8, p, u64, u32, p]),
        "nice_tile_grid": (i, [u32, u32, u32, u32, pu32, pu32]),
        "nice_tiled_bound": (u64, [u32] * 4),
        "nice_tile_select": (i, [u32] * 8 + [pu32] * 4),
        "nice_tiles_split_dev": (i, [p, p, p, u64, u32, u32, u8, u32, u32, p, u64]),
        "nice_tiles_merge_dev": (i, [p, p, p, u64, p, u32, u8] + [u32] * 8 + [u8, u8, p, u64]),
        "nice_encode_tiled_dev": (i, [p, p, p, u64, u32, u32, u8, u8, u32, u32, p, u64, p, p, p, p]),
        "nice_decode_tiled_dev": (i, [p, p, p, u64, p, p, p] + [u32] * 8 + [u8, p, u64, u32, p]),
        "nice_tile_alpha_width": (u32, [u32]),
        "nice_tiled_alpha_bound": (u64, [u32] * 4),
        "nice_tiles_alpha_range_dev": (i, [p, p, p, u64, u32, u32, u32, u32, p, p]),
        "nice_encode_tiled_alpha_dev": (i, [p, p, p, u64, u32, u32, u32, u32, p, u64, p, p, p, p, p]),
        "nice_decode_tiled_alpha_dev": (i, [p, p, p, u64, p, p, p, p] + [u32] * 8 + [p, u64, p]),
        "nice_set_grid": (i, [p, p, u32, u32, u32, p]),
        "nice_set_bound": (u64, [p, p, u32, u32, u32]),
        "nice_set_select": (i, [p, p, u32, u32, u32, p, u32, p]),
        "nice_set_split_dev": (i, [p, p, p, p, p, p, u32, u8, u32, u32, p, u64]),
        "nice_set_merge_dev": (i, [p, p, p, u64, p, p, p, p, u32, u8, p, p, u32, u32, u32, p, p, p, u32, u8, u8]),
        "nice_encode_set_dev": (i, [p, p, p, p, p, p, u32, u8, u8, u32, u32, p, u64, p, p, p, p]),
        "nice_decode_set_dev": (i, [p, p, p, u64, p, p, p, p, p, u32, u32, u32, p, p, p, u32, u8, u32, p]),
        "nice_set_alpha_bound": (u64, [p, p, u32, u32, u32]),
        "nice_set_alpha_range_dev": (i, [p, p, p, p, p, p, u32, u32, u32, p, p]),
        "nice_encode_set_alpha_dev": (i, [p, p, p, p, p, p, u32, u32, u32, p, u64, p, p, p, p, p]),
        "nice_decode_set_alpha_dev": (i, [p, p, p, u64, p, p, p, p, p, p, u32, u32, u32, p, p, p, u32, p]),
        "nice_set_merge_tensor_dev": (i, [p, p, p, u64, p, p, p, p, u32, u8, p, p, u32, u32, u32, p, p, p, p, p, u32,
                                          u32, u32, p, p]),
        "nice_decode_set_tensor_dev": (i, [p, p, p, u64, p, p, p, p, p, u32, u32, u32, p, p, p, p, p, u32, u32, u32, p,
                                           p, u32, p]),
        "nice_set_resize_tensor_dev": (i, [p, p, p, u64, p, p, p, p, p, u32, u32, u32, p, p, u32, u32, p, p, p, u32, u32,
                                           u32, p, p]),
        "nice_decode_set_resized_dev": (i, [p, p, p, u64, p, p, p, p, p, u32, u32, u32, p, p, u32, u32, p, p, p, u32, u32,
                                            u32, p, p, u32, p]),
        "nice_set_resize_aa_tensor_dev": (i, [p, p, p, u64, p, p, p, p, p, u32, u32, u32, p, p, u32, u32, p, p, p, u32,
                                              u32, u32, p, p]),
        "nice_decode_set_resized_aa_dev": (i, [p, p, p, u64, p, p, p, p, p, u32, u32, u32, p, p, u32, u32, p, p, p, u32,
                                               u32, u32, p, p, u32, p]),
        "nice_pipe_create": (i, [i, u32, u32, u8, u32, u32, pp]),
        "nice_pipe_destroy": (None, [p]),
        "nice_pipe_stream_stride": (u64, [p]),
        "nice_pipe_encode": (i, [p, p, u32, u8, p, u64, p]),
        "nice_pipe_decode": (i, [p, p, p, u32, u8, p, u32, p]),
        "nice_pipe_set_checksums": (i, [p, p, p]),
        "nice_subblock_positions_dev": (i, [i, p, u32, u32, u64, u64, p]),
    }


def _check(rc: int, what: str):
    if rc != OK:
        raise NiceError(rc, what)


@dataclass
class Image:
    """image.rs:5-43 -- only width/height/channels are used on the codec path."""
    width: int
    height: int
    channels: int

    @staticmethod
    def new(width: int, height: int, channels: int) -> "Image":
        return Image(width, height, channels)

    def subblock_positions(self, index0: int = 0, count: int | None = None, device: int = 0, out=None):
        """image.rs:45-102 calc_pos_from for indices [index0, index0 + count)
        (default: the whole image), computed on the GPU into an int64 cuda
        tensor (``out`` or a new one); asynchronous on the current stream."""
        import torch
        n = self.width * self.height - index0 if count is None else count
        if out is None:
            out = torch.empty(max(n, 0), dtype=torch.int64, device=f"cuda:{device}")
        if out.numel() < n or out.dtype != torch.int64 or not out.is_contiguous():
            raise NiceError(E_ARG, "out: contiguous int64 with >= count elements")
        rc = lib().nice_subblock_positions_dev(device, _stream_ptr(torch, out.device), self.width, self.height,
                                               index0, n, _p(out))
        _check(rc, "nice_subblock_positions_dev")
        return out

    def calc_pos_from(self, index: int) -> int:
        """image.rs:45-102: raster position of traversal index ``index``."""
        return int(self.subblock_positions(index, 1)[0])


def encode_bound(width: int, height: int) -> int:
    return int(lib().nice_encode_bound(width, height))


def _as_buffer(data):
    """(ctypes pointer, nbytes, keepalive) for bytes / bytearray / numpy / memoryview."""
    mv = memoryview(data).cast("B")
    if mv.readonly:
        buf = (ctypes.c_uint8 * mv.nbytes).from_buffer_copy(mv)
    else:
        buf = (ctypes.c_uint8 * mv.nbytes).from_buffer(mv)
    return ctypes.cast(buf, ctypes.c_void_p), mv.nbytes, buf


def encode_bytes(input_bytes, width: int, height: int, channels: int,
                 channels_out: int | None = None) -> bytes:
    ptr, n, keep = _as_buffer(input_bytes)
    cap = encode_bound(width, height)
    out = (ctypes.c_uint8 * cap)()
    out_len = ctypes.c_size_t()
    co = channels if channels_out is None else channels_out
    rc = lib().nice_encode(ptr, n, width, height, channels, co, out, cap, ctypes.byref(out_len))
    _check(rc, "nice_encode")
    del keep
    return bytes(out[: out_len.value])


def encode(input_bytes, image_header: Image, channels_out: int, output_writer) -> None:
    """code::encode (code.rs:59-64): appends the stream to ``output_writer``
    (a bytearray, or any object with ``write``)."""
    data = encode_bytes(input_bytes, image_header.width, image_header.height,
                        image_header.channels, channels_out)
    if isinstance(output_writer, bytearray):
        output_writer.extend(data)
    else:
        output_writer.write(data)


def decode_bytes(stream, flags: int = DEC_ALPHA_FILL_FF):
    """Returns (pixels: bytes, Image)."""
    ptr, n, keep = _as_buffer(stream)
    w, h, ch = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint8()
    _check(lib().nice_peek_header(ptr, n, ctypes.byref(w), ctypes.byref(h), ctypes.byref(ch)),
           "nice_peek_header")
    cap = w.value * h.value * max(ch.value, 1)
    out = (ctypes.c_uint8 * max(cap, 1))()
    px_len = ctypes.c_size_t()
    rc = lib().nice_decode(ptr, n, out, cap, flags, ctypes.byref(px_len))
    _check(rc, "nice_decode")
    del keep
    return bytes(out[: px_len.value]), Image(w.value, h.value, ch.value)


def decode(image_reader, channels_out: int, output_vec: bytearray) -> Image:
    """code::decode (code.rs:464-468).  ``channels_out`` is accepted and ignored,
    as in the reference (main.rs:88 passes 3; code.rs never reads it).  The
    output replaces ``output_vec``'s contents."""
    del channels_out
    data = image_reader.read() if hasattr(image_reader, "read") else bytes(image_reader)
    px, img = decode_bytes(data)
    output_vec[:] = px
    return img


# ---- device-resident batches (torch tensors on the GPU) ---------------------
class _Ctx:
    def __init__(self, device: int):
        self.ptr = ctypes.c_void_p()
        _check(lib().nice_ctx_create(device, ctypes.byref(self.ptr)), "nice_ctx_create")

    def __del__(self):
        try:
            if self.ptr:
                lib().nice_ctx_destroy(self.ptr)
        except Exception:
            pass


_ctxs: dict = {}


def _ctx(device: int) -> _Ctx:
    if device not in _ctxs:
        _ctxs[device] = _Ctx(device)
    return _ctxs[device]


def _stream_ptr(torch, device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _stream_of(torch, stream, device):
    return ctypes.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr(torch, device)


def _p(t):
    """The address a tensor's data begins at, as the C ABI takes it."""
    return ctypes.c_void_p(t.data_ptr())


def _launch(torch, device, stream, ctx):
    """(context, stream): what every device entry point's arguments begin with."""
    return (ctx or _ctx(device.index or 0)).ptr, _stream_of(torch, stream, device)


def _host_len(host_len, n: int):
    """``host_len`` (n lengths on the host) as the uint64 array the C ABI reads;
    never an empty one."""
    hl = [int(x) for x in host_len]
    if len(hl) != n:   # a short list would be zero padded: lengths the device does not hold
        raise NiceError(E_ARG, f"host_len has {len(hl)} entries for {n} frames")
    return ctypes.cast((ctypes.c_uint64 * max(n, 1))(*hl), ctypes.c_void_p)


class Context(_Ctx):
    """A device context with its own scratch arena: calls on different torch
    streams need different contexts to run concurrently."""


def encode_batch(px, width: int, height: int, channels: int, out, out_len,
                 channels_out: int | None = None, stream=None, ctx: "_Ctx | None" = None) -> None:
    """Encode ``px`` (uint8 cuda tensor [n_frames, W*H*channels]) into ``out``
    (uint8 cuda tensor [n_frames, stride >= encode_bound]); lengths into
    ``out_len`` (int64 cuda tensor [n_frames]).  Asynchronous on the current
    torch stream (or ``stream``: a torch.cuda.Stream)."""
    import torch
    rc = lib().nice_encode_batch_dev(
        *_launch(torch, px.device, stream, ctx), _p(px), px.stride(0), px.shape[0], width, height,
        channels, channels if channels_out is None else channels_out, _p(out), out.stride(0), _p(out_len))
    _check(rc, "nice_encode_batch_dev")


def decode_batch(streams, stream_len, width: int, height: int, out_channels: int, px, status,
                 flags: int = DEC_ALPHA_FILL_FF, stream=None, ctx: "_Ctx | None" = None,
                 host_len=None) -> None:
    """Decode ``streams`` (uint8 cuda [n, stride]) with byte lengths ``stream_len``
    (int64 cuda [n]) into ``px`` (uint8 cuda [n, >= W*H*out_channels]); per-frame
    status codes into ``status`` (int32 cuda [n]).  Asynchronous: returns once
    the work is queued.  ``host_len`` (the same lengths on the host: a sequence,
    numpy array or CPU tensor) spares the call its one device read (the lengths
    size the scratch), so it never waits for earlier work on the stream."""
    import torch
    n = streams.shape[0]
    args = (*_launch(torch, streams.device, stream, ctx), _p(streams), streams.stride(0), _p(stream_len))
    tail = (n, width, height, out_channels, _p(px), px.stride(0), flags, _p(status))
    if host_len is None:
        rc = lib().nice_decode_batch_dev(*args, *tail)
    else:
        rc = lib().nice_decode_batch_dev_hl(*args, _host_len(host_len, n), *tail)
    _check(rc, "nice_decode_batch_dev")


# ---- packed stream batches (include/nice.h, "packed stream batches") --------
def packed_bound(n_frames: int, width: int, height: int) -> int:
    """Worst-case size of a packed batch of ``n_frames`` width x height streams."""
    return int(lib().nice_packed_bound(n_frames, width, height))


def pack_streams(streams, stream_len, packed, off, status, stream=None, ctx: "_Ctx | None" = None) -> None:
    """Compact ``streams`` (uint8 cuda [n, stride], stride a multiple of 4) with
    byte lengths ``stream_len`` (int64 cuda [n]) into ``packed`` (uint8 cuda,
    16-byte aligned): stream f at ``packed[off[f] : off[f] + stream_len[f]]``,
    ``off`` (int64 cuda [n + 1]) written in full, ``off[n]`` the packed size.
    ``status`` (int32 cuda [1]) receives OK, E_CAPACITY (``off[n]`` exceeds
    ``packed.numel()``; nothing is written past it) or E_ARG (a length above
    the stride).  Asynchronous, never waits for the device."""
    import torch
    n = streams.shape[0]
    if stream_len.numel() < n or off.numel() < n + 1:
        raise NiceError(E_ARG, "pack_streams: stream_len needs n entries, off n + 1")
    rc = lib().nice_pack_streams_dev(
        *_launch(torch, streams.device, stream, ctx), _p(streams), streams.stride(0), _p(stream_len), n,
        _p(packed), packed.numel(), _p(off), _p(status))
    _check(rc, "nice_pack_streams_dev")


def encode_batch_packed(px, width: int, height: int, channels: int, packed, off, out_len, status,
                        channels_out: int | None = None, stream=None, ctx: "_Ctx | None" = None) -> None:
    """``encode_batch`` whose streams land packed: ``px`` (uint8 cuda
    [n, W*H*channels]) is encoded into a strided scratch the context owns and
    reuses, then compacted into ``packed`` as by ``pack_streams`` (``off``
    int64 cuda [n + 1], ``out_len`` int64 cuda [n], ``status`` int32 cuda [1]).
    ``packed_bound(n, width, height)`` bytes always suffice; a smaller buffer
    gives E_CAPACITY in ``status`` and the needed size in ``off[n]``."""
    import torch
    n = px.shape[0]
    if out_len.numel() < n or off.numel() < n + 1:
        raise NiceError(E_ARG, "encode_batch_packed: out_len needs n entries, off n + 1")
    rc = lib().nice_encode_batch_packed_dev(
        *_launch(torch, px.device, stream, ctx), _p(px), px.stride(0), n, width, height, channels,
        channels if channels_out is None else channels_out, _p(packed), packed.numel(), _p(off), _p(out_len),
        _p(status))
    _check(rc, "nice_encode_batch_packed_dev")


def decode_batch_packed(packed, off, stream_len, width: int, height: int, out_channels: int, px, status,
                        flags: int = DEC_ALPHA_FILL_FF, stream=None, ctx: "_Ctx | None" = None,
                        host_len=None, packed_bytes: int | None = None) -> None:
    """``decode_batch`` reading the streams in place from ``packed`` (uint8 cuda,
    16-byte aligned): frame i is the stream at ``off[i]`` with ``stream_len[i]``
    bytes (int64 cuda tensors of n entries each; ``off`` may be a whole n + 1
    table, and a gathered subset in any order with repeats decodes those
    frames).  n = ``stream_len.numel()``.  ``packed_bytes`` (default
    ``packed.numel()``) bounds every ``off[i] + stream_len[i]``; a frame past it
    or with an offset that is not a multiple of 16 gets E_ARG in ``status``
    (int32 cuda [n]), the others decode.  ``host_len`` as for ``decode_batch``."""
    import torch
    n = stream_len.numel()
    if off.numel() < n or status.numel() < n:
        raise NiceError(E_ARG, "decode_batch_packed: off and status need one entry per frame")
    if not off.is_contiguous() or not stream_len.is_contiguous():
        raise NiceError(E_ARG, "decode_batch_packed: off and stream_len must be contiguous")
    pb = packed.numel() if packed_bytes is None else int(packed_bytes)
    if pb > packed.numel():
        raise NiceError(E_ARG, "decode_batch_packed: packed_bytes exceeds the buffer")
    hl = None if host_len is None else _host_len(host_len, n)   # (null: the lengths are read from the device)
    rc = lib().nice_decode_packed_dev(
        *_launch(torch, packed.device, stream, ctx), _p(packed), pb, _p(off), _p(stream_len), hl, n, width, height,
        out_channels, _p(px), px.stride(0), flags, _p(status))
    _check(rc, "nice_decode_packed_dev")


# Host-side container of a packed batch: one file, little-endian throughout.
#   header (40 bytes): magic "NICEPACK", u32 version (1), u32 n, u32 width,
#                      u32 height, u32 channels, u32 reserved (0), u64 packed size
#   n x u64 stream lengths, (n + 1) x u64 offsets, then the packed bytes
_PACK_MAGIC = b"NICEPACK"
_PACK_VERSION = 1
_PACK_HEADER = "<8sIIIIIIQ"


def _batch_chunks(who: str, packed, off, stream_len, kind=None, value=None, n=None, pre=""):
    """One batch as every container stores it: ``(n, size, chunks)``, ``size``
    being ``off[n]`` and ``chunks`` the byte strings to write: n x u64 lengths,
    (n + 1) x u64 offsets, n x u8 kinds and n x u8 values where the batch has
    them, each zero-padded to a multiple of 8 bytes, then ``packed[:size]`` (one
    device-to-host copy).  ``n``: the entries the tables must have (default: as
    many as there are lengths).  ``pre`` ("alpha " or none) words the refusals
    (NiceError(E_ARG), in ``who``'s name)."""
    import numpy as np
    lens, offs = (np.asarray(t.detach().cpu().numpy(), dtype=np.int64).reshape(-1) for t in (stream_len, off))
    bytes_ = [np.asarray(t.detach().cpu().numpy(), dtype=np.uint8).reshape(-1) for t in (kind, value) if t is not None]
    n = lens.size if n is None else n
    if lens.size != n or offs.size != n + 1 or any(t.size != n for t in bytes_):
        raise NiceError(E_ARG, f"{who}: {pre}tables do not match: off has {offs.size} entries for {n} "
                               f"{'tiles' if bytes_ else 'streams'}")
    size = int(offs[n])
    if size < 0 or size > packed.numel():
        raise NiceError(E_ARG, f"{who}: {pre}off[n] exceeds the {pre}packed buffer")
    blob = packed.detach().reshape(-1)[:size].cpu().numpy()
    return n, size, ([lens.astype("<u8").tobytes(), offs.astype("<u8").tobytes()]
                     + [t.tobytes() + bytes(-n % 8) for t in bytes_] + [blob.tobytes()])


def _read_batch(fh, bad, n: int, size: int, max_kind=None, raw_len: int = 0, pre="", device=None):
    """Reads one batch of a container, written as by ``_batch_chunks`` (the
    file's size has been checked against ``n`` and ``size``), and validates
    it: the offsets 16-byte aligned from 0 to ``size``, monotone, no stream
    running into the next; the kinds (read where ``max_kind`` is given) at most
    ``max_kind`` and their padding zero; a raw tile (kind 1) of ``raw_len``
    bytes; with ``max_kind`` 2 the values are read too, a constant tile (kind
    2) has no bytes and only a constant tile a value; nothing truncated.
    ``bad(why)`` makes the error, ``pre`` ("alpha " or none) words it.  Returns
    (packed, off, stream_len[, kind[, value]]): uint8 ``packed`` on ``device``
    (None: the CPU), the tables as int64 / int64 / uint8 / uint8 CPU tensors."""
    import numpy as np
    import torch
    kpad = n + (-n % 8)
    lens = np.frombuffer(fh.read(8 * n), "<u8")
    offs = np.frombuffer(fh.read(8 * (n + 1)), "<u8")
    bytes_ = [np.frombuffer(fh.read(kpad), np.uint8) for _ in range((max_kind is not None) + (max_kind == 2))]
    if lens.size != n or offs.size != n + 1 or any(t.size != kpad for t in bytes_):
        raise bad("truncated")
    if offs[0] != 0 or offs[n] != size or (offs % 16).any():
        raise bad(f"{pre}offsets not 16-byte aligned from 0 to the {pre}packed size")
    if (offs[1:] < offs[:-1]).any():
        raise bad(f"{pre}offsets not monotone")
    if (lens > offs[1:] - offs[:-1]).any():
        raise bad(f"one of the {pre}streams overlaps the next")
    if bytes_:
        kinds = bytes_[0][:n]
        if any(t[n:].any() for t in bytes_) or (kinds > max_kind).any():
            raise bad(f"{pre}tile kinds")
        if (lens[kinds == 1] != raw_len).any():
            raise bad(f"raw {pre}tile length")
        if max_kind == 2 and (lens[kinds == 2] != 0).any():
            raise bad(f"constant {pre}tile with a length")
        if max_kind == 2 and bytes_[1][:n][kinds != 2].any():
            raise bad(f"{pre}value of a tile that is not constant")
    blob = np.frombuffer(fh.read(size), np.uint8)
    if blob.size != size:
        raise bad("truncated")
    packed = torch.from_numpy(blob.copy())
    return (packed if device is None else packed.to(device), torch.from_numpy(offs.astype(np.int64)),
            torch.from_numpy(lens.astype(np.int64)), *[torch.from_numpy(t[:n].copy()) for t in bytes_])


def save_packed(path, packed, off, stream_len, width: int, height: int, channels: int) -> None:
    """Write a packed batch (tensors on the GPU or the CPU) to ``path``: one
    device-to-host copy of ``packed[:off[n]]``."""
    import struct
    n, size, chunks = _batch_chunks("save_packed", packed, off, stream_len)
    with open(path, "wb") as fh:
        fh.write(struct.pack(_PACK_HEADER, _PACK_MAGIC, _PACK_VERSION, n, width, height, channels, 0, size))
        fh.writelines(chunks)


def load_packed(path, device=None):
    """Read a ``save_packed`` file: returns ``(packed, off, stream_len, width,
    height, channels)`` with uint8 / int64 / int64 tensors on ``device`` (one
    host-to-device copy of the blob), or on the CPU with ``device=None`` (no
    GPU needed).  A file that is not a consistent packed batch raises
    NiceError(E_FORMAT)."""
    import struct

    def bad(why):
        return NiceError(E_FORMAT, f"load_packed({path}): {why}")

    hsz = struct.calcsize(_PACK_HEADER)
    fsize = os.path.getsize(path)
    with open(path, "rb") as fh:
        head = fh.read(hsz)
        if len(head) < hsz:
            raise bad("truncated header")
        magic, version, n, width, height, channels, _, size = struct.unpack(_PACK_HEADER, head)
        if magic != _PACK_MAGIC:
            raise bad("wrong magic")
        if version != _PACK_VERSION:
            raise bad(f"version {version}")
        if size % 16 or size >= 1 << 62:
            raise bad("packed size")
        if fsize != hsz + 8 * n + 8 * (n + 1) + size:
            raise bad("file size does not match the header")
        packed, off, stream_len = _read_batch(fh, bad, n, size, device=device)
    if device is not None:
        off, stream_len = off.to(device), stream_len.to(device)
    return packed, off, stream_len, width, height, channels


# ---- tiled images (include/nice.h, "tiled images") ---------------------------
# One image as nx * ny independent tiles in one packed batch: a single large
# image decodes on the whole device, a region decodes from the tiles it touches,
# and tiles the format cannot carry are stored raw, so every input round-trips.
# 1024 x 512: of 512 x 512, 1024 x 1024 and 1024 x 512 the fastest to decode and encode and the
# smallest container on a 4K and a 16384 x 16384 frame (tools/bench_tiled.py; DESIGN.md, "Tiled images").
DEFAULT_TILE = (1024, 512)


@dataclass
class TiledAlpha:
    """The alpha batch of a tiled RGBA image (include/nice.h, "tiled images:
    alpha"): ``packed`` (uint8 tensor, where the colour ``packed`` lives) holds
    tile t's alpha at ``off[t] : off[t] + stream_len[t]``; ``kind[t]`` is 0 for
    a NICE stream of the plane's triplet image, 1 for the raw plane and 2 for a
    constant plane of ``value[t]`` (nothing stored).  ``off`` (n + 1, int64),
    ``stream_len`` (n, int64), ``kind`` and ``value`` (n, uint8) are CPU tensors."""
    packed: object
    off: object
    stream_len: object
    kind: object
    value: object

    @property
    def nbytes(self) -> int:
        return int(self.off[-1])


@dataclass
class TiledImage:
    """A tiled image: ``packed`` (uint8 tensor) holds tile t at
    ``off[t] : off[t] + stream_len[t]``; ``kind[t]`` is 0 for a NICE stream of
    the padded tile and 1 for raw RGB.  ``off`` (n + 1, int64), ``stream_len``
    (n, int64) and ``kind`` (n, uint8) are CPU tensors.  ``alpha``: the alpha
    batch (``TiledAlpha``) of an image encoded with ``alpha=True``, else None."""
    width: int
    height: int
    channels: int
    tile_w: int
    tile_h: int
    packed: object
    off: object
    stream_len: object
    kind: object
    alpha: "TiledAlpha | None" = None

    @property
    def nx(self) -> int:
        return -(-self.width // self.tile_w)

    @property
    def ny(self) -> int:
        return -(-self.height // self.tile_h)

    @property
    def nbytes(self) -> int:
        """Bytes of the packed tiles (the container adds its tables)."""
        return int(self.off[-1])


def tile_grid(width: int, height: int, tile_w: int, tile_h: int):
    """(nx, ny) of a tiled image; NiceError(E_ARG) for a geometry outside the limits."""
    nx, ny = ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib().nice_tile_grid(width, height, tile_w, tile_h, ctypes.byref(nx), ctypes.byref(ny)), "nice_tile_grid")
    return nx.value, ny.value


def _u32_args(*vals):
    if any(v < 0 or v >= 1 << 32 for v in vals):
        raise NiceError(E_ARG, "argument outside 32 bits")
    return vals


def tile_select(width: int, height: int, tile_w: int, tile_h: int, x0: int, y0: int, rw: int, rh: int):
    """(tx0, ty0, tx1, ty1): the half-open tile range the rectangle touches;
    NiceError(E_ARG) for an empty rectangle or one that leaves the image."""
    r = [ctypes.c_uint32() for _ in range(4)]
    _check(lib().nice_tile_select(*_u32_args(width, height, tile_w, tile_h, x0, y0, rw, rh),
                                  *[ctypes.byref(v) for v in r]), "nice_tile_select")
    return tuple(v.value for v in r)


def tiled_bound(width: int, height: int, tile_w: int, tile_h: int) -> int:
    """Worst-case packed size of the tiled image (0: bad geometry)."""
    return int(lib().nice_tiled_bound(width, height, tile_w, tile_h))


def _rows_view(t, what):
    """Row pitch in bytes of a [H, W, C] uint8 cuda tensor whose rows may be strided."""
    if t.dim() != 3 or str(t.dtype) != "torch.uint8" or not t.is_cuda:
        raise NiceError(E_ARG, f"{what}: a uint8 cuda tensor [H, W, C]")
    c = t.shape[2]
    if c not in (3, 4) or t.stride(2) != 1 or t.stride(1) != c or (t.shape[0] > 1 and t.stride(0) < t.shape[1] * c):
        raise NiceError(E_ARG, f"{what}: C of 3 or 4, stride(2) == 1, stride(1) == C, rows not overlapping")
    return t.stride(0) if t.shape[0] > 1 else t.shape[1] * c


def tiled_alpha_bound(width: int, height: int, tile_w: int, tile_h: int) -> int:
    """Worst-case packed size of the tiled image's alpha batch (0: bad geometry)."""
    return int(lib().nice_tiled_alpha_bound(width, height, tile_w, tile_h))


def _encode_tables(torch, n: int, dev, value: bool = False):
    """``(tables, status)`` for a tiled or set encode to fill on ``dev``: the
    tables are off (n + 1, int64), stream_len (n, int64), kind (n, uint8) and,
    for an alpha batch, value (n, uint8); ``status`` is the int32 word."""
    tables = [torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)]
    tables += [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2 if value else 1)]
    return tables, torch.full((1,), 99, dtype=torch.int32, device=dev)


def _encode_tail(rc: int, what: str, stream, status, packed, tables, n: int):
    """What follows the launch of a tiled or set encode: the call's and, after
    the wait, the device's verdict in ``what``'s name, then the tables to the
    host.  Returns ``packed[:off[n]]`` (a view) and the host tables, in the
    order the dataclasses take them."""
    _check(rc, what)
    if stream is not None:
        stream.synchronize()
    _check(int(status.cpu()[0]), what)
    host = [t.cpu() for t in tables]
    return (packed[:int(host[0][n])], *host)


def _encode_tiled_alpha(torch, img, pitch, tw, th, n, stream, ctx) -> TiledAlpha:
    h, w, _ = img.shape
    dev = img.device
    packed = torch.empty(tiled_alpha_bound(w, h, tw, th), dtype=torch.uint8, device=dev)
    tables, status = _encode_tables(torch, n, dev, value=True)
    rc = lib().nice_encode_tiled_alpha_dev(*_launch(torch, dev, stream, ctx), _p(img), pitch, w, h, tw, th, _p(packed),
                                           packed.numel(), *map(_p, tables), _p(status))
    trimmed, *host = _encode_tail(rc, "nice_encode_tiled_alpha_dev", stream, status, packed, tables, n)
    # (a copy: the alpha of a mostly opaque image is far smaller than its bound)
    return TiledAlpha(trimmed.clone(), *host)


def encode_tiled(img, tile=None, channels_out: int | None = None, stream=None, ctx: "_Ctx | None" = None,
                 packed=None, alpha: bool = False) -> TiledImage:
    """Encode ``img`` (uint8 cuda tensor [H, W, C], C 3 or 4, rows may be
    strided: ``stride(1) == C``, ``stride(2) == 1``) as tiles of ``tile`` =
    (tile_w, tile_h) pixels (default ``DEFAULT_TILE``).  Every tile is verified
    by decoding it; the few the format cannot carry are stored raw, so
    ``decode_tiled`` returns the input's RGB for every input (alpha is not
    coded).  ``packed`` (optional uint8 cuda buffer, 16-byte aligned) receives
    the tiles; too small a buffer raises NiceError(E_CAPACITY).  The result's
    ``packed`` is trimmed to ``off[n]``.  ``alpha=True`` (a 4-channel image;
    3 channels raise NiceError(E_ARG)) also stores byte +3 of every pixel, as
    the result's ``alpha`` batch: ``decode_tiled`` then returns all four
    channels.  Waits for the device (the tables come back to the host)."""
    import torch
    tw, th = DEFAULT_TILE if tile is None else tile
    pitch = _rows_view(img, "encode_tiled: img")
    h, w, c = img.shape
    if alpha and c != 4:
        raise NiceError(E_ARG, "encode_tiled: alpha=True needs a 4-channel image")
    nx, ny = tile_grid(w, h, tw, th)
    n = nx * ny
    dev = img.device
    if packed is None:
        packed = torch.empty(tiled_bound(w, h, tw, th), dtype=torch.uint8, device=dev)
    tables, status = _encode_tables(torch, n, dev)
    rc = lib().nice_encode_tiled_dev(
        *_launch(torch, dev, stream, ctx), _p(img), pitch, w, h, c, c if channels_out is None else channels_out, tw, th,
        _p(packed), packed.numel(), *map(_p, tables), _p(status))
    timg = TiledImage(w, h, c, tw, th, *_encode_tail(rc, "nice_encode_tiled_dev", stream, status, packed, tables, n))
    if alpha:
        timg.alpha = _encode_tiled_alpha(torch, img, pitch, tw, th, n, stream, ctx)
    return timg


def _host_tables(torch, who: str, batch, n: int, colour_dev=None):
    """The tables of ``batch`` (a TiledImage or an ImageSet, or, with
    ``colour_dev`` the device of the colour batch, its TiledAlpha) as the
    contiguous CPU tensors a decode reads: [off, stream_len, kind], and value
    for an alpha batch.  They must fit the ``n`` tiles and ``batch.packed``,
    which must be on the GPU, an alpha batch's on ``colour_dev``; else
    NiceError(E_ARG) in the name of ``who``, the public function."""
    alpha = colour_dev is not None
    if not batch.packed.is_cuda or (alpha and batch.packed.device != colour_dev):
        raise NiceError(E_ARG, f"{who}: alpha.packed must be on the GPU, with the colour packed" if alpha else
                        f"{who}: packed must be on the GPU (load_tiled / load_set(path, device=...))")
    tables = [batch.off.to("cpu", torch.int64).contiguous(), batch.stream_len.to("cpu", torch.int64).contiguous(),
              batch.kind.to("cpu", torch.uint8).contiguous()]
    if alpha:
        tables.append(batch.value.to("cpu", torch.uint8).contiguous())
    if (tables[0].numel() < n + 1 or any(t.numel() != n for t in tables[1:])
            or int(tables[0][n]) > batch.packed.numel()):
        raise NiceError(E_ARG, f"{who}: {'alpha ' if alpha else ''}tables do not match the {n} tiles")
    return tables


def _alpha_packed(al: TiledAlpha, tables, n: int):
    """(address, bytes) of an alpha batch's packed bytes: null and 0 where every tile is constant."""
    size = int(tables[0][n])
    return (_p(al.packed) if size else None), size


def _decode_tail(stream, passes, out, alpha_field: bool = True):
    """What follows the launches of a tiled or set decode: the wait, one copy
    of each pass's statuses (``passes``: [(entry point, status tensor)], the
    colour pass first), and, if any slot failed, NiceError with ``.statuses``,
    ``.alpha_statuses`` (None without that pass; absent where ``alpha_field``
    is false) and ``.out``.  Returns ``out``."""
    if stream is not None:
        stream.synchronize()
    sts = [status.cpu().tolist() for _, status in passes]
    bad = [s for st in sts for s in st if s != OK]
    if bad:
        err = NiceError(bad[0], f"{' + '.join(what for what, _ in passes)}: {len(bad)} of {sum(map(len, sts))} "
                                "tiles failed")
        err.statuses = sts[0]
        if alpha_field:
            err.alpha_statuses = sts[1] if len(sts) > 1 else None
        err.out = out
        raise err
    return out


def decode_tiled(timg: TiledImage, roi=None, out=None, out_channels: int | None = None,
                 flags: int = DEC_ALPHA_FILL_FF, stream=None, ctx: "_Ctx | None" = None):
    """Decode ``timg`` (``packed`` on the GPU), or its rectangle ``roi`` =
    (x, y, w, h), into a uint8 cuda tensor [rh, rw, out_channels]
    (``out_channels`` defaults to ``out``'s, else the image's channels).  Only
    the tiles the rectangle touches are decoded.  ``out`` may be a row-strided
    view of a larger tensor.  If any tile fails, its pixels of the window are
    left as they were, the other tiles are written, and NiceError is raised
    with ``.statuses`` (one per selected tile, row-major) and ``.out``.  Where
    ``timg.alpha`` is set and the output has 4 channels, a second pass writes
    the stored alpha into byte +3 (``flags``' DEC_ALPHA_FILL_FF is then
    irrelevant); its statuses are the error's ``.alpha_statuses`` (None without
    that pass), and a failed alpha tile keeps what the colour pass wrote there.
    Waits for the device (the statuses come back)."""
    import torch
    x0, y0, rw, rh = (0, 0, timg.width, timg.height) if roi is None else roi
    tw, th = timg.tile_w, timg.tile_h
    tx0, ty0, tx1, ty1 = tile_select(timg.width, timg.height, tw, th, x0, y0, rw, rh)
    nx, ny = tile_grid(timg.width, timg.height, tw, th)
    n = nx * ny
    packed = timg.packed
    tables = _host_tables(torch, "decode_tiled", timg, n)
    dev = packed.device
    if out is None:
        oc = timg.channels if out_channels is None else out_channels
        out = torch.empty((rh, rw, oc), dtype=torch.uint8, device=dev)
    else:
        if out.dim() != 3 or tuple(out.shape[:2]) != (rh, rw) or (out_channels not in (None, out.shape[2])):
            raise NiceError(E_ARG, "decode_tiled: out must be [rh, rw, out_channels]")
        if out.device != dev:
            raise NiceError(E_ARG, "decode_tiled: out on another device")
    pitch = _rows_view(out, "decode_tiled: out")
    m = (tx1 - tx0) * (ty1 - ty0)
    status = torch.full((m,), 99, dtype=torch.int32, device=dev)
    geom = (timg.width, timg.height, tw, th, x0, y0, rw, rh)
    rc = lib().nice_decode_tiled_dev(*_launch(torch, dev, stream, ctx), _p(packed), int(tables[0][n]),
                                     *map(_p, tables), *geom, out.shape[2], _p(out), pitch, flags, _p(status))
    _check(rc, "nice_decode_tiled_dev")
    passes = [("nice_decode_tiled_dev", status)]
    if timg.alpha is not None and out.shape[2] == 4:   # the stored alpha over byte +3 of what the colour pass wrote
        atables = _host_tables(torch, "decode_tiled", timg.alpha, n, colour_dev=dev)
        astatus = torch.full((m,), 99, dtype=torch.int32, device=dev)
        rc = lib().nice_decode_tiled_alpha_dev(
            *_launch(torch, dev, stream, ctx), *_alpha_packed(timg.alpha, atables, n), *map(_p, atables), *geom,
            _p(out), pitch, _p(astatus))
        _check(rc, "nice_decode_tiled_alpha_dev")
        passes.append(("nice_decode_tiled_alpha_dev", astatus))
    return _decode_tail(stream, passes, out)


# Host-side container of a tiled image: one file, little-endian throughout
# (NICEPACK version 1 above is a different file and stays as it is).
#   header (56 bytes): magic "NICETILE", u32 version (1), u32 width, height,
#                      channels, tile_w, tile_h, nx, ny, u32 reserved (0), u64 packed size
#   n x u64 lengths, (n + 1) x u64 offsets, n x u8 kinds zero-padded to a
#   multiple of 8 bytes, then the packed bytes
# An image with an alpha batch is version 2: the reserved word is a flags word
# (bit 0: alpha present), and after the colour packed bytes come
#   u64 alpha packed size, n x u64 alpha lengths, (n + 1) x u64 alpha offsets,
#   n x u8 alpha kinds and n x u8 alpha values, each zero-padded to a multiple
#   of 8 bytes, then the alpha packed bytes
# An image without one is written as version 1, as before.
_TILE_MAGIC = b"NICETILE"
_TILE_VERSION = 1
_TILE_VERSION_ALPHA = 2
_TILE_FLAG_ALPHA = 1
_TILE_HEADER = "<8sIIIIIIIIIQ"


def save_tiled(path, timg: TiledImage) -> None:
    """Write ``timg`` (tensors on the GPU or the CPU) to ``path``."""
    import struct
    al = timg.alpha
    n, size, chunks = _tiles_chunks("save_tiled", timg, timg.nx * timg.ny)
    with open(path, "wb") as fh:
        fh.write(struct.pack(_TILE_HEADER, _TILE_MAGIC, _TILE_VERSION if al is None else _TILE_VERSION_ALPHA,
                             timg.width, timg.height, timg.channels, timg.tile_w, timg.tile_h, timg.nx, timg.ny,
                             0 if al is None else _TILE_FLAG_ALPHA, size))
        fh.writelines(chunks)


def _tiles_chunks(who: str, batch, n: int):
    """``_batch_chunks`` of the n tiles of a TiledImage or an ImageSet; where it
    has an alpha batch, the alpha part of a version 2 container (NICETILE and
    NICESETS alike) follows: the u64 alpha packed size, then its chunks."""
    import struct
    n, size, chunks = _batch_chunks(who, batch.packed, batch.off, batch.stream_len, batch.kind, n=n)
    al = batch.alpha
    if al is not None:
        _, asize, achunks = _batch_chunks(who, al.packed, al.off, al.stream_len, al.kind, al.value, n=n, pre="alpha ")
        chunks += [struct.pack("<Q", asize)] + achunks
    return n, size, chunks


def _read_tiles(fh, bad, fsize: int, start: int, n: int, size: int, tw: int, th: int, has_alpha: bool, device):
    """What follows the header fields of a NICETILE or NICESETS container, from
    byte ``start`` on: the colour batch of n tiles and ``size`` packed bytes,
    which ends a version 1 file, and in a version 2 file the alpha part, read
    and validated as strictly, which must end it.  Returns (packed, off,
    stream_len, kind, alpha), ``alpha`` a TiledAlpha or None."""
    import struct
    kpad = n + (-n % 8)
    colour_end = start + 8 * n + 8 * (n + 1) + kpad + size
    if (fsize < colour_end + 8) if has_alpha else (fsize != colour_end):
        raise bad("file size does not match the header")
    colour = _read_batch(fh, bad, n, size, max_kind=1, raw_len=tw * th * 3, device=device)
    if not has_alpha:
        return (*colour, None)
    (asize,) = struct.unpack("<Q", fh.read(8))
    if asize % 16 or asize >= 1 << 62:
        raise bad("alpha packed size")
    if fsize != colour_end + 8 + 8 * n + 8 * (n + 1) + 2 * kpad + asize:
        raise bad("file size does not match the alpha tables")
    alpha = _read_batch(fh, bad, n, asize, max_kind=2, raw_len=tw * th, pre="alpha ", device=device)
    return (*colour, TiledAlpha(*alpha))


def load_tiled(path, device=None) -> TiledImage:
    """Read a ``save_tiled`` file.  ``packed`` goes to ``device`` (one
    host-to-device copy), or stays on the CPU with ``device=None`` (no GPU and
    no libnice_hip.so needed); the tables are CPU tensors.  A file that is not
    a consistent tiled image raises NiceError(E_FORMAT)."""
    import struct

    def bad(why):
        return NiceError(E_FORMAT, f"load_tiled({path}): {why}")

    hsz = struct.calcsize(_TILE_HEADER)
    fsize = os.path.getsize(path)
    with open(path, "rb") as fh:
        head = fh.read(hsz)
        if len(head) < hsz:
            raise bad("truncated header")
        magic, version, w, h, c, tw, th, nx, ny, reserved, size = struct.unpack(_TILE_HEADER, head)
        if magic != _TILE_MAGIC:
            raise bad("wrong magic")
        if version not in (_TILE_VERSION, _TILE_VERSION_ALPHA):
            raise bad(f"version {version}")
        # version 1: a reserved zero; version 2: the flags, alpha (bit 0) the only one and always set
        has_alpha = version == _TILE_VERSION_ALPHA
        if reserved != (_TILE_FLAG_ALPHA if has_alpha else 0):
            raise bad("flags")
        if c not in (3, 4) or w == 0 or h == 0 or w * h > 1 << 30 or (has_alpha and c != 4):
            raise bad("image size or channels")
        if not (2 <= tw <= 8192 and 2 <= th <= 8192):
            raise bad("tile size")
        if nx != -(-w // tw) or ny != -(-h // th):
            raise bad("grid does not match the image and tile sizes")
        n = nx * ny
        if n * (-(-tw * th // 1024)) >= 1 << 32:
            raise bad("too many tiles")
        if size % 16 or size >= 1 << 62:
            raise bad("packed size")
        return TiledImage(w, h, c, tw, th, *_read_tiles(fh, bad, fsize, hsz, n, size, tw, th, has_alpha, device))


# ---- image sets (include/nice.h, "image sets") --------------------------------
# Many images of different sizes as one packed batch of equally sized tiles:
# one batch encode, one batch decode, whatever the number of images or windows.
# 256 x 256: of 256 x 256, 512 x 512 and 1024 x 512 the fastest to decode and encode and the smallest
# container on 256 images of 256..1536 pixels a side (tools/bench_sets.py; DESIGN.md, "Image sets").
DEFAULT_SET_TILE = (256, 256)


@dataclass
class ImageSet:
    """A set of K images: image i is ``widths[i]`` x ``heights[i]``, its tiles
    are ``first[i] : first[i + 1]`` of the n tiles in ``packed`` (uint8 tensor),
    tile t at ``off[t] : off[t] + stream_len[t]``; ``kind[t]`` is 0 for a NICE
    stream of the padded tile and 1 for raw RGB.  ``widths``, ``heights`` and
    ``first`` (K + 1) are lists; ``off`` (n + 1, int64), ``stream_len`` (n,
    int64) and ``kind`` (n, uint8) are CPU tensors.  ``alpha``: the alpha batch
    (``TiledAlpha``, its tables over the same n global tiles) of a set encoded
    with ``alpha=True``, else None."""
    widths: list
    heights: list
    channels: int
    tile_w: int
    tile_h: int
    first: list
    packed: object
    off: object
    stream_len: object
    kind: object
    alpha: "TiledAlpha | None" = None

    @property
    def nbytes(self) -> int:
        """Bytes of the packed tiles (the container adds its tables)."""
        return int(self.off[-1])

    def __len__(self) -> int:
        return len(self.widths)


def _u32_array(vals):
    vals = [int(v) for v in vals]
    _u32_args(*vals)
    return (ctypes.c_uint32 * max(len(vals), 1))(*vals)


def _set_geom(widths, heights, tile_w: int, tile_h: int):
    """A set's geometry as the C ABI takes it: (h_w, h_h, K, tile_w, tile_h)."""
    return _u32_array(widths), _u32_array(heights), len(widths), tile_w, tile_h


def _images(tensors, pitches):
    """Per-image (or per-window) base addresses and row pitches, as two host arrays."""
    k = len(tensors)
    return (ctypes.c_void_p * k)(*[t.data_ptr() for t in tensors]), (ctypes.c_uint64 * k)(*pitches)


def set_grid(widths, heights, tile_w: int, tile_h: int):
    """``first`` (K + 1 ints): the scan of the images' tile counts, ``first[K]``
    the set's n; NiceError(E_ARG) for an empty set or one outside the limits."""
    if len(heights) != len(widths):
        raise NiceError(E_ARG, "set_grid: widths and heights differ in length")
    _u32_args(tile_w, tile_h)
    first = (ctypes.c_uint32 * (len(widths) + 1))()
    _check(lib().nice_set_grid(*_set_geom(widths, heights, tile_w, tile_h), first), "nice_set_grid")
    return list(first)


def set_bound(widths, heights, tile_w: int, tile_h: int) -> int:
    """Worst-case packed size of the set (0: bad set)."""
    if len(heights) != len(widths):
        return 0
    return int(lib().nice_set_bound(*_set_geom(widths, heights, tile_w, tile_h)))


def set_alpha_bound(widths, heights, tile_w: int, tile_h: int) -> int:
    """Worst-case packed size of the set's alpha batch (0: bad set)."""
    if len(heights) != len(widths):
        return 0
    return int(lib().nice_set_alpha_bound(*_set_geom(widths, heights, tile_w, tile_h)))


def _encode_set_alpha(torch, images, pitches, widths, heights, tw, th, n, stream, ctx) -> TiledAlpha:
    dev = images[0].device
    packed = torch.empty(set_alpha_bound(widths, heights, tw, th), dtype=torch.uint8, device=dev)
    tables, status = _encode_tables(torch, n, dev, value=True)
    rc = lib().nice_encode_set_alpha_dev(
        *_launch(torch, dev, stream, ctx), *_images(images, pitches), *_set_geom(widths, heights, tw, th), _p(packed),
        packed.numel(), *map(_p, tables), _p(status))
    trimmed, *host = _encode_tail(rc, "nice_encode_set_alpha_dev", stream, status, packed, tables, n)
    # (a copy: the alpha of mostly opaque images is far smaller than its bound)
    return TiledAlpha(trimmed.clone(), *host)


def _win_array(windows):
    flat = []
    for wdw in windows:
        if len(wdw) != 5:
            raise NiceError(E_ARG, "a window is (image, x, y, w, h)")
        flat += list(wdw)
    return _u32_array(flat)


def set_select(widths, heights, tile_w: int, tile_h: int, windows):
    """``slot_first`` (M + 1 ints) for ``windows`` = [(image, x, y, w, h), ...]:
    window j's slots, the tiles it touches inside its image in row-major order,
    are ``slot_first[j] : slot_first[j + 1]``.  NiceError(E_ARG) for an image
    index past the set, an empty window or one that leaves its image."""
    m = len(windows)
    if len(heights) != len(widths):
        raise NiceError(E_ARG, "set_select: widths and heights differ in length")
    _u32_args(tile_w, tile_h)
    sf = (ctypes.c_uint32 * (m + 1))()
    _check(lib().nice_set_select(*_set_geom(widths, heights, tile_w, tile_h), _win_array(windows), m, sf),
           "nice_set_select")
    return list(sf)


def encode_set(images, tile=None, channels_out: int | None = None, stream=None, ctx: "_Ctx | None" = None,
               packed=None, alpha: bool = False) -> ImageSet:
    """Encode ``images`` (a list of uint8 cuda tensors [H, W, C] of any sizes,
    one C of 3 or 4 and one device; rows may be strided as for
    ``encode_tiled``) as one set with tiles of ``tile`` = (tile_w, tile_h)
    pixels (default ``DEFAULT_SET_TILE``): one batch encode and verify over the
    tiles of all images.  Tile ``first[i] + t`` equals tile t of
    ``encode_tiled(images[i], tile)``.  ``packed`` (optional uint8 cuda buffer,
    16-byte aligned) receives the tiles; too small a buffer raises
    NiceError(E_CAPACITY).  ``alpha=True`` (4-channel images; 3 channels raise
    NiceError(E_ARG)) also stores byte +3 of every pixel, as the result's
    ``alpha`` batch over the same n tiles (one more batch encode over the
    tiles whose alpha is not constant, whatever the number of images):
    ``decode_set`` then returns all four channels.  Waits for the device (the
    tables come back)."""
    import torch
    tw, th = DEFAULT_SET_TILE if tile is None else tile
    images = list(images)
    if not images:
        raise NiceError(E_ARG, "encode_set: no images")
    pitches = [_rows_view(t, f"encode_set: images[{i}]") for i, t in enumerate(images)]
    c, dev = images[0].shape[2], images[0].device
    if any(t.shape[2] != c or t.device != dev for t in images):
        raise NiceError(E_ARG, "encode_set: the images must share their channels and their device")
    if alpha and c != 4:
        raise NiceError(E_ARG, "encode_set: alpha=True needs 4-channel images")
    widths, heights = [t.shape[1] for t in images], [t.shape[0] for t in images]
    first = set_grid(widths, heights, tw, th)
    n = first[-1]
    if packed is None:
        packed = torch.empty(set_bound(widths, heights, tw, th), dtype=torch.uint8, device=dev)
    tables, status = _encode_tables(torch, n, dev)
    rc = lib().nice_encode_set_dev(   # (the channels stand between K and the tile size)
        *_launch(torch, dev, stream, ctx), *_images(images, pitches), _u32_array(widths), _u32_array(heights),
        len(images), c, c if channels_out is None else channels_out, tw, th, _p(packed), packed.numel(),
        *map(_p, tables), _p(status))
    iset = ImageSet(widths, heights, c, tw, th, first,
                    *_encode_tail(rc, "nice_encode_set_dev", stream, status, packed, tables, n))
    if alpha:
        iset.alpha = _encode_set_alpha(torch, images, pitches, widths, heights, tw, th, n, stream, ctx)
    return iset


def _set_windows(who: str, iset: ImageSet, images, windows):
    """What a set decode is to produce, from its ``images`` / ``windows``
    arguments (not both; neither: every image): ``(windows, m, slot_first, n)``
    with the M windows as int quintuples, their slots (``set_select``) and the
    set's tile count."""
    if images is not None and windows is not None:
        raise NiceError(E_ARG, f"{who}: images or windows, not both")
    k = len(iset.widths)
    if windows is None:
        idx = range(k) if images is None else [int(i) for i in images]
        if any(i < 0 or i >= k for i in idx):
            raise NiceError(E_ARG, f"{who}: image index outside the set")
        windows = [(i, 0, 0, iset.widths[i], iset.heights[i]) for i in idx]
    windows = [tuple(int(v) for v in wdw) for wdw in windows]
    slot_first = set_select(iset.widths, iset.heights, iset.tile_w, iset.tile_h, windows)
    n = set_grid(iset.widths, iset.heights, iset.tile_w, iset.tile_h)[-1]
    return windows, len(windows), slot_first, n


def _set_outputs(out, windows, new, msg: str):
    """``(outs, result)`` of a set decode: the per-window tensors to write and
    what the call returns.  ``out`` None: ``new(window)`` for every window;
    one batch tensor of M windows: its ``out[j]``; else a list of M tensors.
    Another count is NiceError(E_ARG, ``msg``); what each output must look
    like is the caller's to check."""
    m = len(windows)
    if out is None:
        outs = [new(wdw) for wdw in windows]
        return outs, outs
    if hasattr(out, "dim"):
        if out.dim() != 4 or out.shape[0] != m:
            raise NiceError(E_ARG, msg)
        return [out[j] for j in range(m)], out
    outs = list(out)
    if len(outs) != m:
        raise NiceError(E_ARG, msg)
    return outs, out


def decode_set(iset: ImageSet, images=None, windows=None, out=None, out_channels: int | None = None,
               flags: int = DEC_ALPHA_FILL_FF, stream=None, ctx: "_Ctx | None" = None):
    """Decode ``iset`` (``packed`` on the GPU) with one batch decode: all its
    images (the default), the images ``images`` = [i, ...], or the rectangles
    ``windows`` = [(i, x, y, w, h), ...] (not both).  Returns a list of uint8
    cuda tensors [h, w, out_channels], one per image or window, in that order.
    ``out``: a list of such tensors to decode into (rows may be strided), or,
    where all windows share one size, one tensor [M, rh, rw, C] whose
    ``out[j]`` takes window j (the crop batch; ``out`` itself is returned).
    The outputs must not overlap.  Only the tiles the windows touch are
    decoded, a tile touched by two windows once for each.  If a tile fails,
    its pixels are left as they were, the others are written, and NiceError is
    raised with ``.statuses`` (one per window and tile, window after window,
    row-major inside each: ``set_select``) and ``.out``.  Where ``iset.alpha``
    is set and the outputs have 4 channels, a second pass writes the stored
    alpha into byte +3 (``flags``' DEC_ALPHA_FILL_FF is then irrelevant); its
    statuses, slot for slot, are the error's ``.alpha_statuses`` (None without
    that pass), and a failed alpha slot keeps what the colour pass wrote
    there.  Waits for the device (the statuses come back)."""
    import torch
    windows, m, slot_first, n = _set_windows("decode_set", iset, images, windows)
    packed = iset.packed
    tables = _host_tables(torch, "decode_set", iset, n)
    dev = packed.device

    def new(wdw):
        return torch.empty((wdw[4], wdw[3], iset.channels if out_channels is None else out_channels),
                           dtype=torch.uint8, device=dev)

    outs, result = _set_outputs(out, windows, new, "decode_set: out must be [M, rh, rw, out_channels] or a list of M "
                                                   "tensors")
    oc = outs[0].shape[-1] if outs[0].dim() == 3 else 0
    for wdw, o in zip(windows, outs):
        if o.dim() != 3 or tuple(o.shape) != (wdw[4], wdw[3], oc) or out_channels not in (None, oc):
            raise NiceError(E_ARG, "decode_set: every output must be [rh, rw, out_channels] of its window")
        if o.device != dev:
            raise NiceError(E_ARG, "decode_set: out on another device")
    pitches = [_rows_view(o, "decode_set: out") for o in outs]
    geom = _set_geom(iset.widths, iset.heights, iset.tile_w, iset.tile_h)
    status = torch.full((slot_first[m],), 99, dtype=torch.int32, device=dev)
    rc = lib().nice_decode_set_dev(*_launch(torch, dev, stream, ctx), _p(packed), int(tables[0][n]), *map(_p, tables),
                                   *geom, _win_array(windows), *_images(outs, pitches), m, oc, flags, _p(status))
    _check(rc, "nice_decode_set_dev")
    passes = [("nice_decode_set_dev", status)]
    if iset.alpha is not None and oc == 4:   # the stored alpha over byte +3 of what the colour pass wrote
        atables = _host_tables(torch, "decode_set", iset.alpha, n, colour_dev=dev)
        astatus = torch.full((slot_first[m],), 99, dtype=torch.int32, device=dev)
        rc = lib().nice_decode_set_alpha_dev(
            *_launch(torch, dev, stream, ctx), *_alpha_packed(iset.alpha, atables, n), *map(_p, atables), *geom,
            _win_array(windows), *_images(outs, pitches), m, _p(astatus))
        _check(rc, "nice_decode_set_alpha_dev")
        passes.append(("nice_decode_set_alpha_dev", astatus))
    return _decode_tail(stream, passes, result)


def _f32(v) -> float:
    """``v`` rounded to float32 (to nearest even), as a Python float."""
    return ctypes.c_float(float(v)).value


def normalize_affine(mean, std):
    """``(scale, bias)`` for ``decode_set_tensor`` such that an element is
    ``(x / 255 - mean[c]) / std[c]``: ``scale[c] = 1 / (255 * std[c])`` and
    ``bias[c] = -mean[c] / std[c]``, each computed in double and rounded once to
    float32; returned as two triples of Python floats that float32 holds
    exactly.  These float32 constants, not the doubles, define the result:
    an element is ``fmaf(byte, scale[c], bias[c])`` in float32, which may
    differ in the last place from the double expression rounded once."""
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3:
        raise NiceError(E_ARG, "normalize_affine: mean and std have three entries each")
    return (tuple(_f32(1.0 / (255.0 * s)) for s in std), tuple(_f32(-m / s) for m, s in zip(mean, std)))


def _tensor_pitches(t, layout):
    """(row pitch, plane pitch), in elements, of a [3, rh, rw] output read as
    ``layout``, or None where its strides are not that layout's.  (A stride
    over an axis of one element says nothing.)"""
    _, rh, rw = t.shape
    s0, s1, s2 = t.stride()
    if layout == TENSOR_PLANAR:
        return ((s1 if rh > 1 else rw), s0) if rw == 1 or s2 == 1 else None
    return ((s1 if rh > 1 else 3 * rw), 0) if s0 == 1 and (rw == 1 or s2 == 3) else None


def _decode_set_tensor(who: str, entry: str, resized: bool, iset: ImageSet, *, images, windows, size, out, dtype,
                       scale, bias, flip, channels_last: bool, flags: int, stream, ctx):
    """``decode_set_tensor`` (every output has its window's size) and
    ``decode_set_resized`` (``resized``: every output is ``size`` = (oh, ow)),
    whose arguments these are: the checks, each a NiceError(E_ARG) that names
    ``who``, the outputs and their one layout, then the C entry point ``entry``
    and ``decode_set``'s tail."""
    import torch
    dtype = torch.float16 if dtype is None else dtype
    dt = {torch.float32: TENSOR_F32, torch.float16: TENSOR_F16, torch.bfloat16: TENSOR_BF16}.get(dtype)
    if dt is None:
        raise NiceError(E_ARG, f"{who}: dtype must be torch.float32, torch.float16 or torch.bfloat16")
    if resized:
        try:
            oh, ow = (int(v) for v in size)
        except (TypeError, ValueError):
            raise NiceError(E_ARG, f"{who}: size must be (oh, ow)") from None
        if not (1 <= oh <= RESIZE_MAX and 1 <= ow <= RESIZE_MAX):
            raise NiceError(E_ARG, f"{who}: size must be within 1..{RESIZE_MAX} on both axes")
    windows, m, slot_first, n = _set_windows(who, iset, images, windows)
    packed = iset.packed
    tables = _host_tables(torch, who, iset, n)
    scale, bias = [_f32(v) for v in scale], [_f32(v) for v in bias]
    if len(scale) != 3 or len(bias) != 3:
        raise NiceError(E_ARG, f"{who}: scale and bias have three entries each")
    flips = [0] * m if flip is None else [1 if f else 0 for f in flip]
    if len(flips) != m:
        raise NiceError(E_ARG, f"{who}: flip must have one entry per window")
    dev = packed.device

    def new(*shape):   # [..., 3, h, w] in the memory format asked for
        if channels_last:
            return torch.empty(shape[:-3] + shape[-2:] + (3,), dtype=dtype, device=dev).movedim(-1, -3)
        return torch.empty(shape, dtype=dtype, device=dev)

    if not resized:
        shapes = [(3, wdw[4], wdw[3]) for wdw in windows]
        shape_msg = f"{who}: out must be [M, 3, rh, rw] or a list of M tensors [3, rh, rw] of their windows"
    else:
        shapes = [(3, oh, ow)] * m
        shape_msg = f"{who}: out must be [M, 3, oh, ow] or a list of M tensors [3, oh, ow]"
        if out is None:   # one batch tensor
            out = new(m, 3, oh, ow)
    outs, result = _set_outputs(out, windows, lambda wdw: new(3, wdw[4], wdw[3]), shape_msg)
    for shape, o in zip(shapes, outs):
        if not hasattr(o, "dim") or o.dim() != 3 or tuple(o.shape) != shape:
            raise NiceError(E_ARG, shape_msg)
        if o.dtype != dtype or not o.is_cuda or o.device != dev:
            raise NiceError(E_ARG, f"{who}: out must have the dtype asked for, on the set's device")
    # one layout per call: the first that every output's strides fit
    for layout in (TENSOR_PLANAR, TENSOR_INTERLEAVED):
        pitches = [_tensor_pitches(o, layout) for o in outs]
        if all(v is not None for v in pitches):
            break
    else:
        raise NiceError(E_ARG, f"{who}: the outputs' strides must all be planar (innermost 1) or all interleaved "
                               "(channel stride 1, innermost 3)")
    status = torch.full((slot_first[m],), 99, dtype=torch.int32, device=dev)
    rc = getattr(lib(), entry)(
        *_launch(torch, dev, stream, ctx), _p(packed), int(tables[0][n]), *map(_p, tables),
        *_set_geom(iset.widths, iset.heights, iset.tile_w, iset.tile_h), _win_array(windows),
        (ctypes.c_uint8 * m)(*flips), *((ow, oh) if resized else ()), *_images(outs, [v[0] for v in pitches]),
        (ctypes.c_uint64 * m)(*[v[1] for v in pitches]), m, dt, layout, (ctypes.c_float * 3)(*scale),
        (ctypes.c_float * 3)(*bias), flags, _p(status))
    _check(rc, entry)
    return _decode_tail(stream, [(entry, status)], result, alpha_field=False)


def decode_set_tensor(iset: ImageSet, images=None, windows=None, out=None, dtype=None,
                      scale=(1 / 255,) * 3, bias=(0.,) * 3, flip=None, channels_last: bool = False,
                      flags: int = DEC_ALPHA_FILL_FF, stream=None, ctx: "_Ctx | None" = None):
    """``decode_set`` straight into what a model reads: a list of cuda tensors
    [3, h, w] of ``dtype`` (torch.float16, the default, torch.bfloat16 or
    torch.float32), one per image or window (``images`` / ``windows`` as for
    ``decode_set``).  Element (c, y, x) is ``fmaf(b, scale[c], bias[c])`` in
    float32, b being byte +c of the decoded pixel, stored as float32 or rounded
    to nearest even to ``dtype``; ``scale`` and ``bias`` (three numbers each,
    ``normalize_affine`` gives those of a mean and a std) are rounded to
    float32 once, here, and passed on as they are.  The output has three
    channels, always: a 4-channel set decodes its colour, ``iset.alpha`` is not
    read.  ``flip``: M truthy or falsy values, or None; a truthy one mirrors
    its window (output column x takes window column w - 1 - x).
    ``out``: a list of [3, h, w] tensors to decode into, whose rows and planes
    may be strided while the innermost stride is fixed by the layout, or, where
    all windows share one size, one tensor [M, 3, rh, rw] (``out`` itself is
    returned).  The strides decide the layout, one per call: ``stride(3) == 1``
    is planar (NCHW), ``stride(1) == 1 and stride(3) == 3`` interleaved (a
    ``channels_last`` tensor); anything else is NiceError(E_ARG).  The outputs
    must not overlap.  ``channels_last=True`` only chooses the memory format of
    the tensors the function allocates.  The conversion happens in the merge
    kernel: no uint8 image and no float32 temporary exist.  Errors, the
    untouched elements of a failed tile, ``.statuses`` and ``.out`` and the wait
    are ``decode_set``'s."""
    return _decode_set_tensor("decode_set_tensor", "nice_decode_set_tensor_dev", False, iset, images=images,
                              windows=windows, size=None, out=out, dtype=dtype, scale=scale, bias=bias, flip=flip,
                              channels_last=channels_last, flags=flags, stream=stream, ctx=ctx)


def decode_set_resized(iset: ImageSet, windows=None, images=None, size=None, out=None, dtype=None,
                       scale=(1 / 255,) * 3, bias=(0.,) * 3, flip=None, channels_last: bool = False,
                       flags: int = DEC_ALPHA_FILL_FF, stream=None, ctx: "_Ctx | None" = None,
                       antialias: bool = False):
    """``decode_set_tensor`` with every window resampled to one ``size`` =
    (oh, ow), whatever its own size: a random resized crop per window, from the
    packed set to one cuda tensor [M, 3, oh, ow] of ``dtype`` (float16 by
    default) that the call allocates, or ``out``: such a batch tensor or a list
    of M tensors [3, oh, ow], whose strides decide the layout exactly as in
    ``decode_set_tensor``.  ``windows`` / ``images``, ``scale``, ``bias``,
    ``flip``, ``channels_last`` and ``flags`` are ``decode_set_tensor``'s; each
    of ``oh``, ``ow`` is 1..8192.

    The value is defined exactly and compares bit for bit: fixed-point
    bilinear sampling with 8 fractional bits of position, and no antialiasing
    (a strong reduction aliases, as ``interpolate(antialias=False)`` does).
    For an output axis of ``n_out`` elements over a window axis of ``n_in``
    pixels, output index ``x`` samples at the integer ``q`` (in 1/256 pixel;
    integer arithmetic, floor division)::

        t  = ((2x + 1) * n_in * 256 + n_out) // (2 * n_out)
        q  = min(max(t - 128, 0), (n_in - 1) * 256)
        i0 = q >> 8;  f = q & 255;  i1 = min(i0 + (f != 0), n_in - 1)

    Indices are relative to the window and clamp to the window, not the image;
    a mirrored window takes the column position of ``ow - 1 - x``.  With
    (i0, i1, fx) of the column, (j0, j1, fy) of the row and b the byte of
    channel c::

        acc = (256 - fy) * ((256 - fx) * b[j0][i0] + fx * b[j0][i1]) + fy * ((256 - fx) * b[j1][i0] + fx * b[j1][i1])
        v   = fmaf(float32(acc) * 2**-16, scale[c], bias[c])

    in float32 with the one rounding of the fmaf, stored as float32 or rounded
    to nearest even to ``dtype``.  A window of the output's size gives
    ``decode_set_tensor``'s bits; an exact halving gives the mean of each
    2 x 2 block.  The sampling happens in the one merge launch: no uint8 crop
    and no float32 temporary exist, and the number of launches does not depend
    on M.  An element is written iff every tile one of its taps falls in
    decoded; errors, ``.statuses``, ``.out`` and the wait are
    ``decode_set_tensor``'s.

    ``antialias=True`` filters a reducing axis instead of sampling it: the
    triangle filter of support ``n_in / n_out`` that
    ``interpolate(bilinear, antialias=True)`` and PIL's resize apply, in
    integers and as exactly defined.  Each axis is treated separately.  An
    axis with ``n_out >= n_in`` keeps the taps above with the weights
    ``16 * (256 - f)`` on ``i0`` and ``16 * f`` on ``i1`` (in 1/4096; one tap
    where ``f == 0``).  An axis with ``n_out < n_in`` must have
    ``n_in <= 65536`` (``RESIZE_AA_MAX_IN``; else NiceError(E_ARG)); for
    output index ``x`` (mirrored: ``ow - 1 - x``)::

        C = (2x + 1) * n_in;  P_i = (2i + 1) * n_out;  S = 2 * n_in
        r_i = S - |P_i - C|                     the taps: the i with r_i > 0, one run lo..hi inside the window
        W_i = (cum * 8192 + R) // (2 * R)       cum = r_lo + ... + r_i, R = the sum over the run   [(cum * 8192 + R) / (2 * R), floor]
        w_i = W_i - W_(i-1),  W_(lo-1) = 0      sums to 4096 exactly, none negative

    and with column taps (i, w_i), row taps (j, v_j)::

        h[j]  = sum_i w_i * b[j][i]
        acc32 = sum_j v_j * h[j]
        acc   = (acc32 + 128) >> 8
        v     = fmaf(float32(acc) * 2**-16, scale[c], bias[c])

    A window that reduces on neither axis gives the bits of
    ``antialias=False``; an exact halving has the interior weights 512, 1536,
    1536, 512 (the support-2 triangle, not the block mean).  An element is
    written iff every tile its tap rectangle (columns lo..hi by rows lo..hi)
    meets decoded.  The resampling takes two launches whatever M is: the
    weights, computed on the device, and the separable filter."""
    entry = "nice_decode_set_resized_aa_dev" if antialias else "nice_decode_set_resized_dev"
    return _decode_set_tensor("decode_set_resized", entry, True, iset, images=images, windows=windows, size=size,
                              out=out, dtype=dtype, scale=scale, bias=bias, flip=flip, channels_last=channels_last,
                              flags=flags, stream=stream, ctx=ctx)


# Host-side container of an image set: one file, little-endian throughout
# (NICEPACK and NICETILE above are different files and stay as they are).
#   header (48 bytes): magic "NICESETS", u32 version (1), u32 channels, tile_w,
#                      tile_h, K, u32 reserved (0), u64 tile count n, u64 packed size
#   K x (u32 width, u32 height), then, exactly as in NICETILE: n x u64 lengths,
#   (n + 1) x u64 offsets, n x u8 kinds zero-padded to a multiple of 8 bytes,
#   then the packed bytes
# A set with an alpha batch is version 2: the reserved word is a flags word
# (bit 0: alpha present, the only flag and always set), and after the colour
# packed bytes comes the alpha part exactly as in NICETILE version 2 (u64 alpha
# packed size, alpha lengths, offsets, kinds, values, alpha packed bytes).
# A set without one is written as version 1, as before.
_SET_MAGIC = b"NICESETS"
_SET_VERSION = 1
_SET_VERSION_ALPHA = 2
_SET_FLAG_ALPHA = 1
_SET_HEADER = "<8sIIIIIIQQ"


def _set_first(widths, heights, tw, th):
    """The tile scan of a set in plain Python (load_set needs no library)."""
    first = [0]
    for w, h in zip(widths, heights):
        first.append(first[-1] + (-(-int(w) // tw)) * (-(-int(h) // th)))
    return first


def save_set(path, iset: ImageSet) -> None:
    """Write ``iset`` (tensors on the GPU or the CPU) to ``path``."""
    import struct
    import numpy as np
    k, al = len(iset.widths), iset.alpha
    if k == 0 or k != len(iset.heights):
        raise NiceError(E_ARG, f"save_set: no images, or {k} widths for {len(iset.heights)} heights")
    if al is not None and iset.channels != 4:
        raise NiceError(E_ARG, "save_set: an alpha batch needs a 4-channel set")
    n, size, chunks = _tiles_chunks("save_set", iset, _set_first(iset.widths, iset.heights, iset.tile_w,
                                                                 iset.tile_h)[-1])
    with open(path, "wb") as fh:
        fh.write(struct.pack(_SET_HEADER, _SET_MAGIC, _SET_VERSION if al is None else _SET_VERSION_ALPHA,
                             iset.channels, iset.tile_w, iset.tile_h, k, 0 if al is None else _SET_FLAG_ALPHA, n,
                             size))
        fh.write(np.stack([np.asarray(iset.widths, "<u4"), np.asarray(iset.heights, "<u4")], axis=1).tobytes())
        fh.writelines(chunks)


def load_set(path, device=None) -> ImageSet:
    """Read a ``save_set`` file.  ``packed`` goes to ``device`` (one
    host-to-device copy), or stays on the CPU with ``device=None`` (no GPU and
    no libnice_hip.so needed); the tables are CPU tensors.  A file that is not
    a consistent image set raises NiceError(E_FORMAT)."""
    import struct
    import numpy as np

    def bad(why):
        return NiceError(E_FORMAT, f"load_set({path}): {why}")

    hsz = struct.calcsize(_SET_HEADER)
    fsize = os.path.getsize(path)
    with open(path, "rb") as fh:
        head = fh.read(hsz)
        if len(head) < hsz:
            raise bad("truncated header")
        magic, version, c, tw, th, k, reserved, n, size = struct.unpack(_SET_HEADER, head)
        if magic != _SET_MAGIC:
            raise bad("wrong magic")
        if version not in (_SET_VERSION, _SET_VERSION_ALPHA):
            raise bad(f"version {version}")
        # version 1: a reserved zero; version 2: the flags, alpha (bit 0) the only one and always set
        has_alpha = version == _SET_VERSION_ALPHA
        if reserved != (_SET_FLAG_ALPHA if has_alpha else 0):
            raise bad("flags" if has_alpha else "reserved word")
        if c not in (3, 4) or (has_alpha and c != 4):
            raise bad("channels")
        if not (2 <= tw <= 8192 and 2 <= th <= 8192):
            raise bad("tile size")
        if k == 0 or fsize < hsz + 8 * k:
            raise bad("image count")
        if size % 16 or size >= 1 << 62:
            raise bad("packed size")
        dims = np.frombuffer(fh.read(8 * k), "<u4").reshape(k, 2).astype(np.int64)
        widths, heights = dims[:, 0].tolist(), dims[:, 1].tolist()
        if any(w == 0 or h == 0 or w * h > 1 << 30 for w, h in zip(widths, heights)):
            raise bad("image size")
        first = _set_first(widths, heights, tw, th)   # always recomputed from the sizes
        if n != first[k]:
            raise bad("tile count does not match the image and tile sizes")
        if n * (-(-tw * th // 1024)) >= 1 << 32:
            raise bad("too many tiles")
        return ImageSet(widths, heights, c, tw, th, first,
                        *_read_tiles(fh, bad, fsize, hsz + 8 * k, n, size, tw, th, has_alpha, device))


def checksum64(buf) -> int:
    """nice_checksum64 (include/nice.h) of a byte buffer, on the host."""
    import numpy as np
    b = np.frombuffer(bytes(buf), np.uint8) if not hasattr(buf, "dtype") else np.asarray(buf, np.uint8).reshape(-1)
    pad = (-b.size) % 4
    if pad:
        b = np.concatenate([b, np.zeros(pad, np.uint8)])
    w = b.view("<u4").astype(np.uint64)
    with np.errstate(over="ignore"):
        A = int(w.sum(dtype=np.uint64))
        B = int((w * np.arange(1, w.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))
    return (A + 0x9E3779B97F4A7C15 * B) % (1 << 64)


# ---- streamed host pipeline (config 5: H2D / compute / D2H overlapped) ------
def _host_ptr(buf):
    """Address of a host buffer: numpy array, bytearray or CPU torch tensor."""
    if hasattr(buf, "data_ptr"):
        return buf.data_ptr()
    if hasattr(buf, "ctypes"):
        return buf.ctypes.data
    return ctypes.addressof((ctypes.c_uint8 * len(buf)).from_buffer(buf))


class Pipeline:
    """Streamed encode/decode of host frames (include/nice.h ``nice_pipe_*``):
    ``depth`` slots of ``batch`` frames, each with its own HIP stream, so H2D
    copies, kernels and D2H copies of different slots overlap.  Host buffers
    may be pinned (``torch.empty(..., pin_memory=True)``: asynchronous copies)
    or pageable (numpy / bytearray)."""

    def __init__(self, width: int, height: int, channels: int, batch: int = 16, depth: int = 3,
                 device: int = 0):
        self.width, self.height, self.channels = width, height, channels
        self.ptr = ctypes.c_void_p()
        _check(lib().nice_pipe_create(device, width, height, channels, batch, depth,
                                      ctypes.byref(self.ptr)), "nice_pipe_create")
        self.stream_stride = int(lib().nice_pipe_stream_stride(self.ptr))

    def close(self):
        if self.ptr:
            lib().nice_pipe_destroy(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def checksums(self, on: bool = True):
        """From the next call on, encode / decode also record each frame's
        checksum64 (computed on the device; ``last_sums`` after the call)."""
        self._ck = on

    def _sums(self, n, enc):
        if not getattr(self, "_ck", False):
            lib().nice_pipe_set_checksums(self.ptr, None, None)
            return None
        buf = (ctypes.c_uint64 * max(n, 1))()
        _check(lib().nice_pipe_set_checksums(self.ptr, buf if enc else None, None if enc else buf),
               "nice_pipe_set_checksums")
        return buf

    def _sums_done(self, buf, n):
        if buf is not None:
            lib().nice_pipe_set_checksums(self.ptr, None, None)
            self.last_sums = [int(buf[i]) for i in range(n)]

    def encode(self, frames, outs, channels_out: int | None = None):
        """frames[f] -> outs[f] (host buffers of >= stream_stride bytes); returns
        the stream lengths."""
        n = len(frames)
        sums = self._sums(n, True)
        src = (ctypes.c_void_p * max(n, 1))(*[_host_ptr(f) for f in frames])
        dst = (ctypes.c_void_p * max(n, 1))(*[_host_ptr(o) for o in outs])
        caps = [o.numel() if hasattr(o, "numel") else len(o) for o in outs]
        lens = (ctypes.c_uint64 * max(n, 1))()
        co = self.channels if channels_out is None else channels_out
        try:
            rc = lib().nice_pipe_encode(self.ptr, src, n, co, dst, min(caps) if caps else 0, lens)
        finally:   # the pipe must not keep pointing at `sums` once it is freed
            self._sums_done(sums, n)
        _check(rc, "nice_pipe_encode")
        return [int(lens[i]) for i in range(n)]

    def decode(self, streams, lengths, outs, out_channels: int | None = None,
               flags: int = DEC_ALPHA_FILL_FF, raise_on_error: bool = True):
        """streams[f] (lengths[f] bytes) -> outs[f] (W*H*out_channels bytes);
        returns the per-frame statuses.  A frame's error raises NiceError unless
        raise_on_error is False (outs[f] is undefined where status[f] != 0)."""
        n = len(streams)
        sums = self._sums(n, False)
        src = (ctypes.c_void_p * max(n, 1))(*[_host_ptr(s) for s in streams])
        dst = (ctypes.c_void_p * max(n, 1))(*[_host_ptr(o) for o in outs])
        ln = (ctypes.c_uint64 * max(n, 1))(*lengths)
        status = (ctypes.c_int32 * max(n, 1))()
        oc = self.channels if out_channels is None else out_channels
        try:
            rc = lib().nice_pipe_decode(self.ptr, src, ln, n, oc, dst, flags, status)
        finally:
            self._sums_done(sums, n)
        st = [int(status[i]) for i in range(n)]
        if rc != 0 and (raise_on_error or rc not in st):
            _check(rc, "nice_pipe_decode")
        return st
