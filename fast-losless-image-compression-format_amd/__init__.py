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
    "load_set", "DEFAULT_SET_TILE", "decode_set_tensor", "normalize_affine",
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
]
TENSOR_F32, TENSOR_F16, TENSOR_BF16 = 0, 1, 2
TENSOR_PLANAR, TENSOR_INTERLEAVED = 0, 1


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
    u8p = ctypes.c_void_p
    sz = ctypes.c_size_t
    u32 = ctypes.c_uint32
    u64 = ctypes.c_uint64
    L.nice_version.restype = ctypes.c_char_p
    L.nice_encode_bound.restype = sz
    L.nice_encode_bound.argtypes = [u32, u32]
    L.nice_encode.argtypes = [u8p, sz, u32, u32, ctypes.c_uint8, ctypes.c_uint8, u8p, sz,
                              ctypes.POINTER(sz)]
    L.nice_peek_header.argtypes = [u8p, sz, ctypes.POINTER(u32), ctypes.POINTER(u32),
                                   ctypes.POINTER(ctypes.c_uint8)]
    L.nice_decode.argtypes = [u8p, sz, u8p, sz, u32, ctypes.POINTER(sz)]
    L.nice_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.nice_ctx_destroy.argtypes = [ctypes.c_void_p]
    L.nice_ctx_reserve.argtypes = [ctypes.c_void_p, u32, u32, u32]
    L.nice_encode_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, u32, u32, u32,
                                        ctypes.c_uint8, ctypes.c_uint8, u8p, u64, u8p]
    L.nice_decode_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, u8p, u32, u32,
                                        u32, ctypes.c_uint8, u8p, u64, u32, u8p]
    L.nice_decode_batch_dev_hl.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, u8p, ctypes.c_void_p, u32,
                                           u32, u32, ctypes.c_uint8, u8p, u64, u32, u8p]
    L.nice_packed_bound.restype = u64
    L.nice_packed_bound.argtypes = [u32, u32, u32]
    L.nice_pack_streams_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, u8p, u32, u8p, u64, u8p, u8p]
    L.nice_encode_batch_packed_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, u32, u32, u32,
                                               ctypes.c_uint8, ctypes.c_uint8, u8p, u64, u8p, u8p, u8p]
    L.nice_decode_packed_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, u8p, u8p, ctypes.c_void_p,
                                         u32, u32, u32, ctypes.c_uint8, u8p, u64, u32, u8p]
    u8 = ctypes.c_uint8
    u32p = ctypes.POINTER(u32)
    L.nice_tile_grid.argtypes = [u32, u32, u32, u32, u32p, u32p]
    L.nice_tiled_bound.restype = u64
    L.nice_tiled_bound.argtypes = [u32, u32, u32, u32]
    L.nice_tile_select.argtypes = [u32] * 8 + [u32p] * 4
    L.nice_tiles_split_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, u32, u32, u8, u32, u32, u8p, u64]
    L.nice_tiles_merge_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, u8p, u32, u8, u32, u32, u32, u32,
                                       u32, u32, u32, u32, u8, u8, u8p, u64]
    L.nice_encode_tiled_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, u32, u32, u8, u8, u32, u32, u8p,
                                        u64, u8p, u8p, u8p, u8p]
    L.nice_decode_tiled_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, u32, u32, u32, u32, u32, u32, u32, u32, u8, u8p, u64, u32,
                                        u8p]
    L.nice_tile_alpha_width.restype = u32
    L.nice_tile_alpha_width.argtypes = [u32]
    L.nice_tiled_alpha_bound.restype = u64
    L.nice_tiled_alpha_bound.argtypes = [u32, u32, u32, u32]
    L.nice_tiles_alpha_range_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, u32, u32, u32, u32, u8p, u8p]
    L.nice_encode_tiled_alpha_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, u32, u32, u32, u32, u8p, u64,
                                              u8p, u8p, u8p, u8p, u8p]
    L.nice_decode_tiled_alpha_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u8p, u64, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, u32, u32, u32, u32, u32,
                                              u32, u32, u32, u8p, u64, u8p]
    vp = ctypes.c_void_p
    L.nice_set_grid.argtypes = [vp, vp, u32, u32, u32, vp]
    L.nice_set_bound.restype = u64
    L.nice_set_bound.argtypes = [vp, vp, u32, u32, u32]
    L.nice_set_select.argtypes = [vp, vp, u32, u32, u32, vp, u32, vp]
    L.nice_set_split_dev.argtypes = [vp, vp, vp, vp, vp, vp, u32, u8, u32, u32, u8p, u64]
    L.nice_set_merge_dev.argtypes = [vp, vp, u8p, u64, vp, vp, vp, vp, u32, u8, vp, vp, u32, u32, u32, vp, vp, vp, u32,
                                     u8, u8]
    L.nice_encode_set_dev.argtypes = [vp, vp, vp, vp, vp, vp, u32, u8, u8, u32, u32, u8p, u64, u8p, u8p, u8p, u8p]
    L.nice_decode_set_dev.argtypes = [vp, vp, u8p, u64, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, u32, u8, u32,
                                      u8p]
    L.nice_set_alpha_bound.restype = u64
    L.nice_set_alpha_bound.argtypes = [vp, vp, u32, u32, u32]
    L.nice_set_alpha_range_dev.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, u32, u8p, u8p]
    L.nice_encode_set_alpha_dev.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, u32, u8p, u64, u8p, u8p, u8p, u8p, u8p]
    L.nice_decode_set_alpha_dev.argtypes = [vp, vp, u8p, u64, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, u32,
                                            u8p]
    L.nice_set_merge_tensor_dev.argtypes = [vp, vp, u8p, u64, vp, vp, vp, vp, u32, u8, vp, vp, u32, u32, u32, vp, vp, vp,
                                            vp, vp, u32, u32, u32, vp, vp]
    L.nice_decode_set_tensor_dev.argtypes = [vp, vp, u8p, u64, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, u32,
                                             u32, u32, vp, vp, u32, u8p]
    L.nice_pipe_create.argtypes = [ctypes.c_int, u32, u32, ctypes.c_uint8, u32, u32,
                                   ctypes.POINTER(ctypes.c_void_p)]
    L.nice_pipe_destroy.argtypes = [ctypes.c_void_p]
    L.nice_pipe_stream_stride.restype = u64
    L.nice_pipe_stream_stride.argtypes = [ctypes.c_void_p]
    L.nice_pipe_encode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u32, ctypes.c_uint8,
                                   ctypes.c_void_p, u64, ctypes.c_void_p]
    L.nice_pipe_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, u32,
                                   ctypes.c_uint8, ctypes.c_void_p, u32, ctypes.c_void_p]
    L.nice_pipe_set_checksums.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.nice_subblock_positions_dev.argtypes = [ctypes.c_int, ctypes.c_void_p, u32, u32, u64, u64,
                                              ctypes.c_void_p]
    _lib = L
    return L


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
                                               index0, n, ctypes.c_void_p(out.data_ptr()))
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
    dev = px.device.index or 0
    n = px.shape[0]
    st = ctypes.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr(torch, px.device)
    rc = lib().nice_encode_batch_dev(
        (ctx or _ctx(dev)).ptr, st, ctypes.c_void_p(px.data_ptr()), px.stride(0), n, width, height,
        channels, channels if channels_out is None else channels_out,
        ctypes.c_void_p(out.data_ptr()), out.stride(0), ctypes.c_void_p(out_len.data_ptr()))
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
    dev = streams.device.index or 0
    n = streams.shape[0]
    st = ctypes.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr(torch, streams.device)
    args = ((ctx or _ctx(dev)).ptr, st, ctypes.c_void_p(streams.data_ptr()), streams.stride(0),
            ctypes.c_void_p(stream_len.data_ptr()))
    tail = (n, width, height, out_channels, ctypes.c_void_p(px.data_ptr()), px.stride(0), flags,
            ctypes.c_void_p(status.data_ptr()))
    if host_len is None:
        rc = lib().nice_decode_batch_dev(*args, *tail)
    else:
        hl_list = [int(x) for x in host_len]
        if len(hl_list) != n:   # a short list would be zero padded: lengths the device does not hold
            raise NiceError(E_ARG, f"host_len has {len(hl_list)} entries for {n} frames")
        hl = (ctypes.c_uint64 * n)(*hl_list)
        rc = lib().nice_decode_batch_dev_hl(*args, ctypes.cast(hl, ctypes.c_void_p), *tail)
    _check(rc, "nice_decode_batch_dev")


# ---- packed stream batches (include/nice.h, "packed stream batches") --------
def packed_bound(n_frames: int, width: int, height: int) -> int:
    """Worst-case size of a packed batch of ``n_frames`` width x height streams."""
    return int(lib().nice_packed_bound(n_frames, width, height))


def _stream_of(torch, stream, device):
    return ctypes.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr(torch, device)


def pack_streams(streams, stream_len, packed, off, status, stream=None, ctx: "_Ctx | None" = None) -> None:
    """Compact ``streams`` (uint8 cuda [n, stride], stride a multiple of 4) with
    byte lengths ``stream_len`` (int64 cuda [n]) into ``packed`` (uint8 cuda,
    16-byte aligned): stream f at ``packed[off[f] : off[f] + stream_len[f]]``,
    ``off`` (int64 cuda [n + 1]) written in full, ``off[n]`` the packed size.
    ``status`` (int32 cuda [1]) receives OK, E_CAPACITY (``off[n]`` exceeds
    ``packed.numel()``; nothing is written past it) or E_ARG (a length above
    the stride).  Asynchronous, never waits for the device."""
    import torch
    dev = streams.device.index or 0
    n = streams.shape[0]
    if stream_len.numel() < n or off.numel() < n + 1:
        raise NiceError(E_ARG, "pack_streams: stream_len needs n entries, off n + 1")
    rc = lib().nice_pack_streams_dev(
        (ctx or _ctx(dev)).ptr, _stream_of(torch, stream, streams.device), ctypes.c_void_p(streams.data_ptr()),
        streams.stride(0), ctypes.c_void_p(stream_len.data_ptr()), n,
        ctypes.c_void_p(packed.data_ptr()), packed.numel(), ctypes.c_void_p(off.data_ptr()),
        ctypes.c_void_p(status.data_ptr()))
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
    dev = px.device.index or 0
    n = px.shape[0]
    if out_len.numel() < n or off.numel() < n + 1:
        raise NiceError(E_ARG, "encode_batch_packed: out_len needs n entries, off n + 1")
    rc = lib().nice_encode_batch_packed_dev(
        (ctx or _ctx(dev)).ptr, _stream_of(torch, stream, px.device), ctypes.c_void_p(px.data_ptr()), px.stride(0),
        n, width, height, channels, channels if channels_out is None else channels_out,
        ctypes.c_void_p(packed.data_ptr()), packed.numel(), ctypes.c_void_p(off.data_ptr()),
        ctypes.c_void_p(out_len.data_ptr()), ctypes.c_void_p(status.data_ptr()))
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
    dev = packed.device.index or 0
    n = stream_len.numel()
    if off.numel() < n or status.numel() < n:
        raise NiceError(E_ARG, "decode_batch_packed: off and status need one entry per frame")
    if not off.is_contiguous() or not stream_len.is_contiguous():
        raise NiceError(E_ARG, "decode_batch_packed: off and stream_len must be contiguous")
    pb = packed.numel() if packed_bytes is None else int(packed_bytes)
    if pb > packed.numel():
        raise NiceError(E_ARG, "decode_batch_packed: packed_bytes exceeds the buffer")
    hl = None
    if host_len is not None:
        hl_list = [int(x) for x in host_len]
        if len(hl_list) != n:
            raise NiceError(E_ARG, f"host_len has {len(hl_list)} entries for {n} frames")
        hl = ctypes.cast((ctypes.c_uint64 * max(n, 1))(*hl_list), ctypes.c_void_p)
    rc = lib().nice_decode_packed_dev(
        (ctx or _ctx(dev)).ptr, _stream_of(torch, stream, packed.device), ctypes.c_void_p(packed.data_ptr()), pb,
        ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(stream_len.data_ptr()), hl, n, width, height,
        out_channels, ctypes.c_void_p(px.data_ptr()), px.stride(0), flags, ctypes.c_void_p(status.data_ptr()))
    _check(rc, "nice_decode_packed_dev")


# Host-side container of a packed batch: one file, little-endian throughout.
#   header (40 bytes): magic "NICEPACK", u32 version (1), u32 n, u32 width,
#                      u32 height, u32 channels, u32 reserved (0), u64 packed size
#   n x u64 stream lengths, (n + 1) x u64 offsets, then the packed bytes
_PACK_MAGIC = b"NICEPACK"
_PACK_VERSION = 1
_PACK_HEADER = "<8sIIIIIIQ"


def save_packed(path, packed, off, stream_len, width: int, height: int, channels: int) -> None:
    """Write a packed batch (tensors on the GPU or the CPU) to ``path``: one
    device-to-host copy of ``packed[:off[n]]``."""
    import struct
    import numpy as np
    lens = np.asarray(stream_len.detach().cpu().numpy(), dtype=np.int64).reshape(-1)
    n = lens.size
    offs = np.asarray(off.detach().cpu().numpy(), dtype=np.int64).reshape(-1)
    if offs.size != n + 1:
        raise NiceError(E_ARG, f"save_packed: off has {offs.size} entries for {n} streams")
    size = int(offs[n])
    if size < 0 or size > packed.numel():
        raise NiceError(E_ARG, "save_packed: off[n] exceeds the packed buffer")
    blob = packed.detach().reshape(-1)[:size].cpu().numpy()
    with open(path, "wb") as fh:
        fh.write(struct.pack(_PACK_HEADER, _PACK_MAGIC, _PACK_VERSION, n, width, height, channels, 0, size))
        fh.write(lens.astype("<u8").tobytes())
        fh.write(offs.astype("<u8").tobytes())
        fh.write(blob.tobytes())


def load_packed(path, device=None):
    """Read a ``save_packed`` file: returns ``(packed, off, stream_len, width,
    height, channels)`` with uint8 / int64 / int64 tensors on ``device`` (one
    host-to-device copy of the blob), or on the CPU with ``device=None`` (no
    GPU needed).  A file that is not a consistent packed batch raises
    NiceError(E_FORMAT)."""
    import struct
    import numpy as np
    import torch

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
        lens = np.frombuffer(fh.read(8 * n), "<u8")
        offs = np.frombuffer(fh.read(8 * (n + 1)), "<u8")
        if offs[0] != 0 or offs[n] != size or (offs % 16).any():
            raise bad("offsets not 16-byte aligned from 0 to the packed size")
        if (offs[1:] < offs[:-1]).any():
            raise bad("offsets not monotone")
        if (lens > offs[1:] - offs[:-1]).any():
            raise bad("a stream overlaps the next")
        blob = np.frombuffer(fh.read(size), np.uint8)
        if blob.size != size:
            raise bad("truncated")
    packed = torch.from_numpy(blob.copy())
    off = torch.from_numpy(offs.astype(np.int64))
    stream_len = torch.from_numpy(lens.astype(np.int64))
    if device is not None:
        packed, off, stream_len = packed.to(device), off.to(device), stream_len.to(device)
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


def _encode_tiled_alpha(torch, img, pitch, tw, th, n, stream, ctx) -> TiledAlpha:
    h, w, _ = img.shape
    dev = img.device
    packed = torch.empty(tiled_alpha_bound(w, h, tw, th), dtype=torch.uint8, device=dev)
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    lens = torch.empty(n, dtype=torch.int64, device=dev)
    kind = torch.empty(n, dtype=torch.uint8, device=dev)
    val = torch.empty(n, dtype=torch.uint8, device=dev)
    status = torch.full((1,), 99, dtype=torch.int32, device=dev)
    rc = lib().nice_encode_tiled_alpha_dev(
        (ctx or _ctx(dev.index or 0)).ptr, _stream_of(torch, stream, dev), ctypes.c_void_p(img.data_ptr()), pitch,
        w, h, tw, th, ctypes.c_void_p(packed.data_ptr()), packed.numel(), ctypes.c_void_p(off.data_ptr()),
        ctypes.c_void_p(lens.data_ptr()), ctypes.c_void_p(kind.data_ptr()), ctypes.c_void_p(val.data_ptr()),
        ctypes.c_void_p(status.data_ptr()))
    _check(rc, "nice_encode_tiled_alpha_dev")
    if stream is not None:
        stream.synchronize()
    _check(int(status.cpu()[0]), "nice_encode_tiled_alpha_dev")
    off_h = off.cpu()
    # (a copy: the alpha of a mostly opaque image is far smaller than its bound)
    return TiledAlpha(packed[:int(off_h[n])].clone(), off_h, lens.cpu(), kind.cpu(), val.cpu())


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
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    lens = torch.empty(n, dtype=torch.int64, device=dev)
    kind = torch.empty(n, dtype=torch.uint8, device=dev)
    status = torch.full((1,), 99, dtype=torch.int32, device=dev)
    rc = lib().nice_encode_tiled_dev(
        (ctx or _ctx(dev.index or 0)).ptr, _stream_of(torch, stream, dev), ctypes.c_void_p(img.data_ptr()), pitch,
        w, h, c, c if channels_out is None else channels_out, tw, th, ctypes.c_void_p(packed.data_ptr()),
        packed.numel(), ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(lens.data_ptr()),
        ctypes.c_void_p(kind.data_ptr()), ctypes.c_void_p(status.data_ptr()))
    _check(rc, "nice_encode_tiled_dev")
    if stream is not None:
        stream.synchronize()
    _check(int(status.cpu()[0]), "nice_encode_tiled_dev")
    off_h = off.cpu()
    timg = TiledImage(w, h, c, tw, th, packed[:int(off_h[n])], off_h, lens.cpu(), kind.cpu())
    if alpha:
        timg.alpha = _encode_tiled_alpha(torch, img, pitch, tw, th, n, stream, ctx)
    return timg


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
    if not packed.is_cuda:
        raise NiceError(E_ARG, "decode_tiled: timg.packed must be on the GPU (load_tiled(path, device=...))")
    off = timg.off.to("cpu", torch.int64).contiguous()
    lens = timg.stream_len.to("cpu", torch.int64).contiguous()
    kind = timg.kind.to("cpu", torch.uint8).contiguous()
    if off.numel() < n + 1 or lens.numel() != n or kind.numel() != n or int(off[n]) > packed.numel():
        raise NiceError(E_ARG, "decode_tiled: tables do not match the grid")
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
    rc = lib().nice_decode_tiled_dev(
        (ctx or _ctx(dev.index or 0)).ptr, _stream_of(torch, stream, dev), ctypes.c_void_p(packed.data_ptr()),
        int(off[n]), ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(lens.data_ptr()),
        ctypes.c_void_p(kind.data_ptr()), timg.width, timg.height, tw, th, x0, y0, rw, rh, out.shape[2],
        ctypes.c_void_p(out.data_ptr()), pitch, flags, ctypes.c_void_p(status.data_ptr()))
    _check(rc, "nice_decode_tiled_dev")
    al = timg.alpha if out.shape[2] == 4 else None
    if al is not None:   # the stored alpha over byte +3 of what the colour pass wrote
        if not al.packed.is_cuda or al.packed.device != dev:
            raise NiceError(E_ARG, "decode_tiled: timg.alpha.packed must be on the GPU, with timg.packed")
        aoff = al.off.to("cpu", torch.int64).contiguous()
        alens = al.stream_len.to("cpu", torch.int64).contiguous()
        akind = al.kind.to("cpu", torch.uint8).contiguous()
        aval = al.value.to("cpu", torch.uint8).contiguous()
        if (aoff.numel() < n + 1 or alens.numel() != n or akind.numel() != n or aval.numel() != n
                or int(aoff[n]) > al.packed.numel()):
            raise NiceError(E_ARG, "decode_tiled: alpha tables do not match the grid")
        astatus = torch.full((m,), 99, dtype=torch.int32, device=dev)
        rc = lib().nice_decode_tiled_alpha_dev(
            (ctx or _ctx(dev.index or 0)).ptr, _stream_of(torch, stream, dev),
            ctypes.c_void_p(al.packed.data_ptr() if int(aoff[n]) else None), int(aoff[n]),
            ctypes.c_void_p(aoff.data_ptr()), ctypes.c_void_p(alens.data_ptr()), ctypes.c_void_p(akind.data_ptr()),
            ctypes.c_void_p(aval.data_ptr()), timg.width, timg.height, tw, th, x0, y0, rw, rh,
            ctypes.c_void_p(out.data_ptr()), pitch, ctypes.c_void_p(astatus.data_ptr()))
        _check(rc, "nice_decode_tiled_alpha_dev")
    if stream is not None:
        stream.synchronize()
    st = status.cpu().tolist()
    ast = astatus.cpu().tolist() if al is not None else None
    bad = [s for s in st + (ast or []) if s != OK]
    if bad:
        what = "nice_decode_tiled_dev" if al is None else "nice_decode_tiled_dev + nice_decode_tiled_alpha_dev"
        err = NiceError(bad[0], f"{what}: {len(bad)} of {m if al is None else 2 * m} tiles failed")
        err.statuses = st
        err.alpha_statuses = ast
        err.out = out
        raise err
    return out


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
    import numpy as np
    n = timg.nx * timg.ny
    lens = np.asarray(timg.stream_len.detach().cpu().numpy(), dtype=np.int64).reshape(-1)
    offs = np.asarray(timg.off.detach().cpu().numpy(), dtype=np.int64).reshape(-1)
    kinds = np.asarray(timg.kind.detach().cpu().numpy(), dtype=np.uint8).reshape(-1)
    if lens.size != n or offs.size != n + 1 or kinds.size != n:
        raise NiceError(E_ARG, f"save_tiled: tables do not match the {timg.nx} x {timg.ny} grid")
    size = int(offs[n])
    if size < 0 or size > timg.packed.numel():
        raise NiceError(E_ARG, "save_tiled: off[n] exceeds the packed buffer")
    blob = timg.packed.detach().reshape(-1)[:size].cpu().numpy()
    al = timg.alpha
    if al is not None:
        apart = _alpha_part(al, n, "save_tiled")
    with open(path, "wb") as fh:
        fh.write(struct.pack(_TILE_HEADER, _TILE_MAGIC, _TILE_VERSION if al is None else _TILE_VERSION_ALPHA,
                             timg.width, timg.height, timg.channels, timg.tile_w, timg.tile_h, timg.nx, timg.ny,
                             0 if al is None else _TILE_FLAG_ALPHA, size))
        fh.write(lens.astype("<u8").tobytes())
        fh.write(offs.astype("<u8").tobytes())
        fh.write(kinds.tobytes() + bytes(-n % 8))
        fh.write(blob.tobytes())
        if al is not None:
            fh.write(apart)


def _alpha_part(al: TiledAlpha, n: int, who: str) -> bytes:
    """The alpha part of a version 2 container (NICETILE and NICESETS alike)."""
    import struct
    import numpy as np
    alens = np.asarray(al.stream_len.detach().cpu().numpy(), dtype=np.int64).reshape(-1)
    aoffs = np.asarray(al.off.detach().cpu().numpy(), dtype=np.int64).reshape(-1)
    akinds = np.asarray(al.kind.detach().cpu().numpy(), dtype=np.uint8).reshape(-1)
    avals = np.asarray(al.value.detach().cpu().numpy(), dtype=np.uint8).reshape(-1)
    if alens.size != n or aoffs.size != n + 1 or akinds.size != n or avals.size != n:
        raise NiceError(E_ARG, f"{who}: alpha tables do not match the {n} tiles")
    asize = int(aoffs[n])
    if asize < 0 or asize > al.packed.numel():
        raise NiceError(E_ARG, f"{who}: alpha off[n] exceeds the alpha packed buffer")
    ablob = al.packed.detach().reshape(-1)[:asize].cpu().numpy()
    return b"".join([struct.pack("<Q", asize), alens.astype("<u8").tobytes(), aoffs.astype("<u8").tobytes(),
                     akinds.tobytes() + bytes(-n % 8), avals.tobytes() + bytes(-n % 8), ablob.tobytes()])


def _load_alpha_part(fh, fsize: int, start: int, n: int, tw: int, th: int, bad, device) -> TiledAlpha:
    """Reads and validates, as strictly as the colour tables, the alpha part
    that begins at byte ``start`` of a version 2 container and must end the file."""
    import struct
    import numpy as np
    import torch
    kpad = n + (-n % 8)
    (asize,) = struct.unpack("<Q", fh.read(8))
    if asize % 16 or asize >= 1 << 62:
        raise bad("alpha packed size")
    if fsize != start + 8 + 8 * n + 8 * (n + 1) + 2 * kpad + asize:
        raise bad("file size does not match the alpha tables")
    alens = np.frombuffer(fh.read(8 * n), "<u8")
    aoffs = np.frombuffer(fh.read(8 * (n + 1)), "<u8")
    akinds = np.frombuffer(fh.read(kpad), np.uint8)
    avals = np.frombuffer(fh.read(kpad), np.uint8)
    if aoffs[0] != 0 or aoffs[n] != asize or (aoffs % 16).any():
        raise bad("alpha offsets not 16-byte aligned from 0 to the alpha packed size")
    if (aoffs[1:] < aoffs[:-1]).any():
        raise bad("alpha offsets not monotone")
    if (alens > aoffs[1:] - aoffs[:-1]).any():
        raise bad("an alpha tile overlaps the next")
    if akinds[n:].any() or avals[n:].any() or (akinds[:n] > 2).any():
        raise bad("alpha tile kinds")
    if (alens[akinds[:n] == 1] != tw * th).any():
        raise bad("raw alpha tile length")
    if (alens[akinds[:n] == 2] != 0).any():
        raise bad("constant alpha tile with a length")
    if avals[:n][akinds[:n] != 2].any():
        raise bad("alpha value of a tile that is not constant")
    ablob = np.frombuffer(fh.read(asize), np.uint8)
    if ablob.size != asize:
        raise bad("truncated")
    apacked = torch.from_numpy(ablob.copy())
    return TiledAlpha(apacked if device is None else apacked.to(device),
                      torch.from_numpy(aoffs.astype(np.int64)), torch.from_numpy(alens.astype(np.int64)),
                      torch.from_numpy(akinds[:n].copy()), torch.from_numpy(avals[:n].copy()))


def load_tiled(path, device=None) -> TiledImage:
    """Read a ``save_tiled`` file.  ``packed`` goes to ``device`` (one
    host-to-device copy), or stays on the CPU with ``device=None`` (no GPU and
    no libnice_hip.so needed); the tables are CPU tensors.  A file that is not
    a consistent tiled image raises NiceError(E_FORMAT)."""
    import struct
    import numpy as np
    import torch

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
        kpad = n + (-n % 8)
        colour_end = hsz + 8 * n + 8 * (n + 1) + kpad + size
        if (fsize < colour_end + 8) if has_alpha else (fsize != colour_end):
            raise bad("file size does not match the header")
        lens = np.frombuffer(fh.read(8 * n), "<u8")
        offs = np.frombuffer(fh.read(8 * (n + 1)), "<u8")
        kinds = np.frombuffer(fh.read(kpad), np.uint8)
        if lens.size != n or offs.size != n + 1 or kinds.size != kpad:
            raise bad("truncated")
        if offs[0] != 0 or offs[n] != size or (offs % 16).any():
            raise bad("offsets not 16-byte aligned from 0 to the packed size")
        if (offs[1:] < offs[:-1]).any():
            raise bad("offsets not monotone")
        if (lens > offs[1:] - offs[:-1]).any():
            raise bad("a tile overlaps the next")
        if kinds[n:].any() or (kinds[:n] > 1).any():
            raise bad("tile kinds")
        if (lens[kinds[:n] == 1] != tw * th * 3).any():
            raise bad("raw tile length")
        blob = np.frombuffer(fh.read(size), np.uint8)
        if blob.size != size:
            raise bad("truncated")
        alpha = None
        if has_alpha:
            alpha = _load_alpha_part(fh, fsize, colour_end, n, tw, th, bad, device)
    packed = torch.from_numpy(blob.copy())
    if device is not None:
        packed = packed.to(device)
    return TiledImage(w, h, c, tw, th, packed, torch.from_numpy(offs.astype(np.int64)),
                      torch.from_numpy(lens.astype(np.int64)), torch.from_numpy(kinds[:n].copy()), alpha)


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


def set_grid(widths, heights, tile_w: int, tile_h: int):
    """``first`` (K + 1 ints): the scan of the images' tile counts, ``first[K]``
    the set's n; NiceError(E_ARG) for an empty set or one outside the limits."""
    k = len(widths)
    if len(heights) != k:
        raise NiceError(E_ARG, "set_grid: widths and heights differ in length")
    _u32_args(tile_w, tile_h)
    first = (ctypes.c_uint32 * (k + 1))()
    _check(lib().nice_set_grid(_u32_array(widths), _u32_array(heights), k, tile_w, tile_h, first), "nice_set_grid")
    return list(first)


def set_bound(widths, heights, tile_w: int, tile_h: int) -> int:
    """Worst-case packed size of the set (0: bad set)."""
    if len(heights) != len(widths):
        return 0
    return int(lib().nice_set_bound(_u32_array(widths), _u32_array(heights), len(widths), tile_w, tile_h))


def set_alpha_bound(widths, heights, tile_w: int, tile_h: int) -> int:
    """Worst-case packed size of the set's alpha batch (0: bad set)."""
    if len(heights) != len(widths):
        return 0
    return int(lib().nice_set_alpha_bound(_u32_array(widths), _u32_array(heights), len(widths), tile_w, tile_h))


def _encode_set_alpha(torch, images, pitches, widths, heights, tw, th, n, stream, ctx) -> TiledAlpha:
    k, dev = len(images), images[0].device
    packed = torch.empty(set_alpha_bound(widths, heights, tw, th), dtype=torch.uint8, device=dev)
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    lens = torch.empty(n, dtype=torch.int64, device=dev)
    kind = torch.empty(n, dtype=torch.uint8, device=dev)
    val = torch.empty(n, dtype=torch.uint8, device=dev)
    status = torch.full((1,), 99, dtype=torch.int32, device=dev)
    rc = lib().nice_encode_set_alpha_dev(
        (ctx or _ctx(dev.index or 0)).ptr, _stream_of(torch, stream, dev),
        (ctypes.c_void_p * k)(*[t.data_ptr() for t in images]), (ctypes.c_uint64 * k)(*pitches),
        _u32_array(widths), _u32_array(heights), k, tw, th, ctypes.c_void_p(packed.data_ptr()), packed.numel(),
        ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(lens.data_ptr()), ctypes.c_void_p(kind.data_ptr()),
        ctypes.c_void_p(val.data_ptr()), ctypes.c_void_p(status.data_ptr()))
    _check(rc, "nice_encode_set_alpha_dev")
    if stream is not None:
        stream.synchronize()
    _check(int(status.cpu()[0]), "nice_encode_set_alpha_dev")
    off_h = off.cpu()
    # (a copy: the alpha of mostly opaque images is far smaller than its bound)
    return TiledAlpha(packed[:int(off_h[n])].clone(), off_h, lens.cpu(), kind.cpu(), val.cpu())


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
    k, m = len(widths), len(windows)
    if len(heights) != k:
        raise NiceError(E_ARG, "set_select: widths and heights differ in length")
    _u32_args(tile_w, tile_h)
    sf = (ctypes.c_uint32 * (m + 1))()
    _check(lib().nice_set_select(_u32_array(widths), _u32_array(heights), k, tile_w, tile_h, _win_array(windows), m,
                                 sf), "nice_set_select")
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
    k, n = len(images), first[-1]
    if packed is None:
        packed = torch.empty(set_bound(widths, heights, tw, th), dtype=torch.uint8, device=dev)
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    lens = torch.empty(n, dtype=torch.int64, device=dev)
    kind = torch.empty(n, dtype=torch.uint8, device=dev)
    status = torch.full((1,), 99, dtype=torch.int32, device=dev)
    rc = lib().nice_encode_set_dev(
        (ctx or _ctx(dev.index or 0)).ptr, _stream_of(torch, stream, dev),
        (ctypes.c_void_p * k)(*[t.data_ptr() for t in images]), (ctypes.c_uint64 * k)(*pitches),
        _u32_array(widths), _u32_array(heights), k, c, c if channels_out is None else channels_out, tw, th,
        ctypes.c_void_p(packed.data_ptr()), packed.numel(), ctypes.c_void_p(off.data_ptr()),
        ctypes.c_void_p(lens.data_ptr()), ctypes.c_void_p(kind.data_ptr()), ctypes.c_void_p(status.data_ptr()))
    _check(rc, "nice_encode_set_dev")
    if stream is not None:
        stream.synchronize()
    _check(int(status.cpu()[0]), "nice_encode_set_dev")
    off_h = off.cpu()
    iset = ImageSet(widths, heights, c, tw, th, first, packed[:int(off_h[n])], off_h, lens.cpu(), kind.cpu())
    if alpha:
        iset.alpha = _encode_set_alpha(torch, images, pitches, widths, heights, tw, th, n, stream, ctx)
    return iset


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
    if images is not None and windows is not None:
        raise NiceError(E_ARG, "decode_set: images or windows, not both")
    k = len(iset.widths)
    tw, th = iset.tile_w, iset.tile_h
    if windows is None:
        idx = range(k) if images is None else [int(i) for i in images]
        if any(i < 0 or i >= k for i in idx):
            raise NiceError(E_ARG, "decode_set: image index outside the set")
        windows = [(i, 0, 0, iset.widths[i], iset.heights[i]) for i in idx]
    windows = [tuple(int(v) for v in wdw) for wdw in windows]
    m = len(windows)
    slot_first = set_select(iset.widths, iset.heights, tw, th, windows)
    first = set_grid(iset.widths, iset.heights, tw, th)
    n = first[-1]
    packed = iset.packed
    if not packed.is_cuda:
        raise NiceError(E_ARG, "decode_set: iset.packed must be on the GPU (load_set(path, device=...))")
    off = iset.off.to("cpu", torch.int64).contiguous()
    lens = iset.stream_len.to("cpu", torch.int64).contiguous()
    kind = iset.kind.to("cpu", torch.uint8).contiguous()
    if off.numel() < n + 1 or lens.numel() != n or kind.numel() != n or int(off[n]) > packed.numel():
        raise NiceError(E_ARG, "decode_set: tables do not match the set")
    dev = packed.device
    result = out
    if out is None:
        oc = iset.channels if out_channels is None else out_channels
        outs = result = [torch.empty((wdw[4], wdw[3], oc), dtype=torch.uint8, device=dev) for wdw in windows]
    elif hasattr(out, "dim"):
        if out.dim() != 4 or out.shape[0] != m:
            raise NiceError(E_ARG, "decode_set: out must be [M, rh, rw, out_channels] or a list of M tensors")
        outs = [out[j] for j in range(m)]
    else:
        outs = list(out)
        if len(outs) != m:
            raise NiceError(E_ARG, "decode_set: out must be [M, rh, rw, out_channels] or a list of M tensors")
    oc = outs[0].shape[-1] if outs[0].dim() == 3 else 0
    for wdw, o in zip(windows, outs):
        if o.dim() != 3 or tuple(o.shape) != (wdw[4], wdw[3], oc) or out_channels not in (None, oc):
            raise NiceError(E_ARG, "decode_set: every output must be [rh, rw, out_channels] of its window")
        if o.device != dev:
            raise NiceError(E_ARG, "decode_set: out on another device")
    pitches = [_rows_view(o, "decode_set: out") for o in outs]
    status = torch.full((slot_first[m],), 99, dtype=torch.int32, device=dev)
    rc = lib().nice_decode_set_dev(
        (ctx or _ctx(dev.index or 0)).ptr, _stream_of(torch, stream, dev), ctypes.c_void_p(packed.data_ptr()),
        int(off[n]), ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(lens.data_ptr()),
        ctypes.c_void_p(kind.data_ptr()), _u32_array(iset.widths), _u32_array(iset.heights), k, tw, th,
        _win_array(windows), (ctypes.c_void_p * m)(*[o.data_ptr() for o in outs]), (ctypes.c_uint64 * m)(*pitches), m,
        oc, flags, ctypes.c_void_p(status.data_ptr()))
    _check(rc, "nice_decode_set_dev")
    al = iset.alpha if oc == 4 else None
    if al is not None:   # the stored alpha over byte +3 of what the colour pass wrote
        if not al.packed.is_cuda or al.packed.device != dev:
            raise NiceError(E_ARG, "decode_set: iset.alpha.packed must be on the GPU, with iset.packed")
        aoff = al.off.to("cpu", torch.int64).contiguous()
        alens = al.stream_len.to("cpu", torch.int64).contiguous()
        akind = al.kind.to("cpu", torch.uint8).contiguous()
        aval = al.value.to("cpu", torch.uint8).contiguous()
        if (aoff.numel() < n + 1 or alens.numel() != n or akind.numel() != n or aval.numel() != n
                or int(aoff[n]) > al.packed.numel()):
            raise NiceError(E_ARG, "decode_set: alpha tables do not match the set")
        astatus = torch.full((slot_first[m],), 99, dtype=torch.int32, device=dev)
        rc = lib().nice_decode_set_alpha_dev(
            (ctx or _ctx(dev.index or 0)).ptr, _stream_of(torch, stream, dev),
            ctypes.c_void_p(al.packed.data_ptr() if int(aoff[n]) else None), int(aoff[n]),
            ctypes.c_void_p(aoff.data_ptr()), ctypes.c_void_p(alens.data_ptr()), ctypes.c_void_p(akind.data_ptr()),
            ctypes.c_void_p(aval.data_ptr()), _u32_array(iset.widths), _u32_array(iset.heights), k, tw, th,
            _win_array(windows), (ctypes.c_void_p * m)(*[o.data_ptr() for o in outs]), (ctypes.c_uint64 * m)(*pitches),
            m, ctypes.c_void_p(astatus.data_ptr()))
        _check(rc, "nice_decode_set_alpha_dev")
    if stream is not None:
        stream.synchronize()
    st = status.cpu().tolist()
    ast = astatus.cpu().tolist() if al is not None else None
    bad = [s for s in st + (ast or []) if s != OK]
    if bad:
        what = "nice_decode_set_dev" if al is None else "nice_decode_set_dev + nice_decode_set_alpha_dev"
        err = NiceError(bad[0], f"{what}: {len(bad)} of {len(st) + len(ast or [])} tiles failed")
        err.statuses = st
        err.alpha_statuses = ast
        err.out = result
        raise err
    return result


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
    import torch
    dtype = torch.float16 if dtype is None else dtype
    dt = {torch.float32: TENSOR_F32, torch.float16: TENSOR_F16, torch.bfloat16: TENSOR_BF16}.get(dtype)
    if dt is None:
        raise NiceError(E_ARG, "decode_set_tensor: dtype must be torch.float32, torch.float16 or torch.bfloat16")
    if images is not None and windows is not None:
        raise NiceError(E_ARG, "decode_set_tensor: images or windows, not both")
    k = len(iset.widths)
    tw, th = iset.tile_w, iset.tile_h
    if windows is None:
        idx = range(k) if images is None else [int(i) for i in images]
        if any(i < 0 or i >= k for i in idx):
            raise NiceError(E_ARG, "decode_set_tensor: image index outside the set")
        windows = [(i, 0, 0, iset.widths[i], iset.heights[i]) for i in idx]
    windows = [tuple(int(v) for v in wdw) for wdw in windows]
    m = len(windows)
    slot_first = set_select(iset.widths, iset.heights, tw, th, windows)
    n = set_grid(iset.widths, iset.heights, tw, th)[-1]
    packed = iset.packed
    if not packed.is_cuda:
        raise NiceError(E_ARG, "decode_set_tensor: iset.packed must be on the GPU (load_set(path, device=...))")
    off = iset.off.to("cpu", torch.int64).contiguous()
    lens = iset.stream_len.to("cpu", torch.int64).contiguous()
    kind = iset.kind.to("cpu", torch.uint8).contiguous()
    if off.numel() < n + 1 or lens.numel() != n or kind.numel() != n or int(off[n]) > packed.numel():
        raise NiceError(E_ARG, "decode_set_tensor: tables do not match the set")
    scale, bias = [_f32(v) for v in scale], [_f32(v) for v in bias]
    if len(scale) != 3 or len(bias) != 3:
        raise NiceError(E_ARG, "decode_set_tensor: scale and bias have three entries each")
    flips = [0] * m if flip is None else [1 if f else 0 for f in flip]
    if len(flips) != m:
        raise NiceError(E_ARG, "decode_set_tensor: flip must have one entry per window")
    dev = packed.device
    result = out
    shape_msg = "decode_set_tensor: out must be [M, 3, rh, rw] or a list of M tensors [3, rh, rw] of their windows"
    if out is None:
        if channels_last:
            outs = [torch.empty((wdw[4], wdw[3], 3), dtype=dtype, device=dev).permute(2, 0, 1) for wdw in windows]
        else:
            outs = [torch.empty((3, wdw[4], wdw[3]), dtype=dtype, device=dev) for wdw in windows]
        result = outs
    elif hasattr(out, "dim"):
        if out.dim() != 4 or out.shape[0] != m:
            raise NiceError(E_ARG, shape_msg)
        outs = [out[j] for j in range(m)]
    else:
        outs = list(out)
        if len(outs) != m:
            raise NiceError(E_ARG, shape_msg)
    for wdw, o in zip(windows, outs):
        if not hasattr(o, "dim") or o.dim() != 3 or tuple(o.shape) != (3, wdw[4], wdw[3]):
            raise NiceError(E_ARG, shape_msg)
        if o.dtype != dtype or not o.is_cuda or o.device != dev:
            raise NiceError(E_ARG, "decode_set_tensor: out must have the dtype asked for, on the set's device")
    # one layout per call: the first that every output's strides fit
    for layout in (TENSOR_PLANAR, TENSOR_INTERLEAVED):
        pitches = [_tensor_pitches(o, layout) for o in outs]
        if all(v is not None for v in pitches):
            break
    else:
        raise NiceError(E_ARG, "decode_set_tensor: the outputs' strides must all be planar (innermost 1) or all "
                               "interleaved (channel stride 1, innermost 3)")
    status = torch.full((slot_first[m],), 99, dtype=torch.int32, device=dev)
    rc = lib().nice_decode_set_tensor_dev(
        (ctx or _ctx(dev.index or 0)).ptr, _stream_of(torch, stream, dev), ctypes.c_void_p(packed.data_ptr()),
        int(off[n]), ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(lens.data_ptr()),
        ctypes.c_void_p(kind.data_ptr()), _u32_array(iset.widths), _u32_array(iset.heights), k, tw, th,
        _win_array(windows), (ctypes.c_uint8 * m)(*flips), (ctypes.c_void_p * m)(*[o.data_ptr() for o in outs]),
        (ctypes.c_uint64 * m)(*[v[0] for v in pitches]), (ctypes.c_uint64 * m)(*[v[1] for v in pitches]), m,
        dt, layout, (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias), flags,
        ctypes.c_void_p(status.data_ptr()))
    _check(rc, "nice_decode_set_tensor_dev")
    if stream is not None:
        stream.synchronize()
    st = status.cpu().tolist()
    bad = [s for s in st if s != OK]
    if bad:
        err = NiceError(bad[0], f"nice_decode_set_tensor_dev: {len(bad)} of {len(st)} tiles failed")
        err.statuses = st
        err.out = result
        raise err
    return result


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
    k = len(iset.widths)
    n = _set_first(iset.widths, iset.heights, iset.tile_w, iset.tile_h)[-1] if k == len(iset.heights) else -1
    lens = np.asarray(iset.stream_len.detach().cpu().numpy(), dtype=np.int64).reshape(-1)
    offs = np.asarray(iset.off.detach().cpu().numpy(), dtype=np.int64).reshape(-1)
    kinds = np.asarray(iset.kind.detach().cpu().numpy(), dtype=np.uint8).reshape(-1)
    if k == 0 or lens.size != n or offs.size != n + 1 or kinds.size != n:
        raise NiceError(E_ARG, f"save_set: tables do not match the {k} images")
    size = int(offs[n])
    if size < 0 or size > iset.packed.numel():
        raise NiceError(E_ARG, "save_set: off[n] exceeds the packed buffer")
    blob = iset.packed.detach().reshape(-1)[:size].cpu().numpy()
    al = iset.alpha
    if al is not None:
        if iset.channels != 4:
            raise NiceError(E_ARG, "save_set: an alpha batch needs a 4-channel set")
        apart = _alpha_part(al, n, "save_set")
    with open(path, "wb") as fh:
        fh.write(struct.pack(_SET_HEADER, _SET_MAGIC, _SET_VERSION if al is None else _SET_VERSION_ALPHA,
                             iset.channels, iset.tile_w, iset.tile_h, k, 0 if al is None else _SET_FLAG_ALPHA, n,
                             size))
        fh.write(np.stack([np.asarray(iset.widths, "<u4"), np.asarray(iset.heights, "<u4")], axis=1).tobytes())
        fh.write(lens.astype("<u8").tobytes())
        fh.write(offs.astype("<u8").tobytes())
        fh.write(kinds.tobytes() + bytes(-n % 8))
        fh.write(blob.tobytes())
        if al is not None:
            fh.write(apart)


def load_set(path, device=None) -> ImageSet:
    """Read a ``save_set`` file.  ``packed`` goes to ``device`` (one
    host-to-device copy), or stays on the CPU with ``device=None`` (no GPU and
    no libnice_hip.so needed); the tables are CPU tensors.  A file that is not
    a consistent image set raises NiceError(E_FORMAT)."""
    import struct
    import numpy as np
    import torch

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
        kpad = n + (-n % 8)
        colour_end = hsz + 8 * k + 8 * n + 8 * (n + 1) + kpad + size
        if (fsize < colour_end + 8) if has_alpha else (fsize != colour_end):
            raise bad("file size does not match the header")
        lens = np.frombuffer(fh.read(8 * n), "<u8")
        offs = np.frombuffer(fh.read(8 * (n + 1)), "<u8")
        kinds = np.frombuffer(fh.read(kpad), np.uint8)
        if lens.size != n or offs.size != n + 1 or kinds.size != kpad:
            raise bad("truncated")
        if offs[0] != 0 or offs[n] != size or (offs % 16).any():
            raise bad("offsets not 16-byte aligned from 0 to the packed size")
        if (offs[1:] < offs[:-1]).any():
            raise bad("offsets not monotone")
        if (lens > offs[1:] - offs[:-1]).any():
            raise bad("a tile overlaps the next")
        if kinds[n:].any() or (kinds[:n] > 1).any():
            raise bad("tile kinds")
        if (lens[kinds[:n] == 1] != tw * th * 3).any():
            raise bad("raw tile length")
        blob = np.frombuffer(fh.read(size), np.uint8)
        if blob.size != size:
            raise bad("truncated")
        alpha = _load_alpha_part(fh, fsize, colour_end, n, tw, th, bad, device) if has_alpha else None
    packed = torch.from_numpy(blob.copy())
    if device is not None:
        packed = packed.to(device)
    return ImageSet(widths, heights, c, tw, th, first, packed, torch.from_numpy(offs.astype(np.int64)),
                    torch.from_numpy(lens.astype(np.int64)), torch.from_numpy(kinds[:n].copy()), alpha)


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
