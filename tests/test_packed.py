"""Packed stream batches (include/nice.h, "packed stream batches"): streams
back to back in one device buffer at 16-byte aligned offsets.

The pack is checked against a numpy packing of the layout on random bytes (it
must not care what it copies); the packed encode against the strided one and
the oracle; the packed decode against the strided decode on every parse route,
on subsets in any order, and on offsets it has to refuse."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY = -1, -4


def _np_pack(src, lens):
    """The layout written out: off[f + 1] = off[f] + align16(len[f]), pads zero."""
    lens = np.asarray(lens, np.int64)
    off = np.zeros(lens.size + 1, np.int64)
    np.cumsum((lens + 15) // 16 * 16, out=off[1:])
    out = np.zeros(int(off[-1]), np.uint8)
    for f, l in enumerate(lens):
        out[off[f]:off[f] + l] = src[f, :l]
    return out, off


def _lengths(n, stride, small):
    """Every residue mod 16 and the edges; `small`: all <= 48 (many streams)."""
    rng = np.random.default_rng(n * 7919 + stride)
    if small:
        lens = rng.integers(0, 49, n)
        lens[:49] = np.arange(49)
        return rng.permutation(lens).astype(np.int64)
    edges = [0, 1, 15, 16, 17, 4095, 4096, 4097, stride] + [32 + r for r in range(16)] + [2048 + r for r in range(16)]
    if n == 1:
        return np.array([stride], np.int64)
    if n == 2:
        return np.array([4097, stride], np.int64)
    lens = rng.integers(0, stride + 1, n)
    lens[:len(edges)] = edges
    return rng.permutation(lens).astype(np.int64)


def _strided(torch, n, stride, base_off):
    """Random bytes in n slots of `stride` bytes, the first `base_off` bytes past a 16-byte boundary."""
    raw = torch.empty(n * stride + 16, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 0
    view = raw[base_off:base_off + n * stride].view(n, stride)
    view.copy_(torch.randint(0, 256, (n, stride), dtype=torch.uint8, device="cuda"))
    assert view.data_ptr() % 16 == base_off
    return raw, view


# (stride of the large-stream cases, stride of the many-small-streams cases, base offset)
LAYOUTS = {"stride256": (4352, 256, 0), "stride4": (5000, 52, 0), "base4": (4352, 256, 4)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [1, 2, 65, 1025, 70000])
def test_pack_matches_numpy(nice, n, layout):
    import torch
    big, small_stride, base_off = LAYOUTS[layout]
    small = n > 65
    stride = small_stride if small else big
    lens = _lengths(n, stride, small)
    assert lens.max() <= stride and (n < 49 or len(set(int(l) % 16 for l in lens)) == 16)
    raw, src = _strided(torch, n, stride, base_off)
    want, want_off = _np_pack(src.cpu().numpy(), lens)
    total = int(want_off[-1])
    packed = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    nice.pack_streams(src, torch.from_numpy(lens).cuda(), packed, off, status)
    torch.cuda.synchronize()
    assert int(status[0]) == 0
    assert np.array_equal(off.cpu().numpy(), want_off)
    got = packed.cpu().numpy()
    assert np.array_equal(got[:total], want)
    assert (got[total:] == 0xA5).all()


def test_pack_single_lengths(nice):
    """One stream of each edge length (n = 1: the wave that holds everything)."""
    import torch
    stride = 5000
    raw, src = _strided(torch, 1, stride, 4)
    host = src.cpu().numpy()
    for l in (0, 1, 15, 16, 17, 4095, 4096, 4097, stride):
        want, want_off = _np_pack(host, [l])
        packed = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        off = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        nice.pack_streams(src, torch.tensor([l], dtype=torch.int64, device="cuda"), packed, off, status)
        torch.cuda.synchronize()
        got = packed.cpu().numpy()
        assert int(status[0]) == 0 and off.tolist() == want_off.tolist(), l
        assert np.array_equal(got[:len(want)], want) and (got[len(want):] == 0xA5).all(), l


def test_pack_capacity(nice):
    import torch
    n, stride = 65, 5000
    lens = _lengths(n, stride, False)
    raw, src = _strided(torch, n, stride, 0)
    want, want_off = _np_pack(src.cpu().numpy(), lens)
    total = int(want_off[-1])
    d_lens = torch.from_numpy(lens).cuda()
    for cap, code in ((total - 16, E_CAPACITY), (total // 2 // 16 * 16, E_CAPACITY), (total, 0)):
        buf = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        nice.pack_streams(src, d_lens, buf[:cap], off, status)
        torch.cuda.synchronize()
        assert int(status[0]) == code, cap
        assert np.array_equal(off.cpu().numpy(), want_off), cap
        got = buf.cpu().numpy()
        assert (got[cap:] == 0xA5).all(), cap
        whole = 0
        for f in range(n):
            if want_off[f] + lens[f] <= cap:
                assert np.array_equal(got[want_off[f]:want_off[f + 1]], want[want_off[f]:want_off[f + 1]]), (cap, f)
                whole += 1
        assert whole >= n // 4, (cap, whole)


# ---- encode / decode through the packed form --------------------------------
class Batch:
    """n frames encoded both ways, built once per module and left unchanged."""

    def __init__(self, nice, O, n, w, h, c):
        import torch
        self.n, self.w, self.h, self.c = n, w, h, c
        self.frames = np.stack([O.gen_syn_v1(w, h, c, s) for s in range(1, n + 1)])
        self.px = torch.from_numpy(self.frames).cuda()
        self.oracle = [O.encode(self.frames[f], w, h, c) for f in range(n)]
        bound = (nice.encode_bound(w, h) + 255) // 256 * 256
        self.strided = torch.zeros((n, bound), dtype=torch.uint8, device="cuda")
        self.lens = torch.zeros(n, dtype=torch.int64, device="cuda")
        nice.encode_batch(self.px, w, h, c, self.strided, self.lens)
        self.packed = torch.full((nice.packed_bound(n, w, h),), 0xA5, dtype=torch.uint8, device="cuda")
        self.off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.plens = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
        nice.encode_batch_packed(self.px, w, h, c, self.packed, self.off, self.plens, self.status)
        torch.cuda.synchronize()
        self.total = int(self.off[n])

    def rgb(self):
        return self.px.view(self.n, -1, self.c)[:, :, :3]

    def decode(self, nice, packed, out_channels, flags, host_len=None, off=None, lens=None, packed_bytes=None,
               data=None):
        import torch
        lens = self.lens if lens is None else lens
        m = lens.numel()
        dec = torch.zeros((m, self.w * self.h * out_channels), dtype=torch.uint8, device="cuda")
        status = torch.full((m,), 99, dtype=torch.int32, device="cuda")
        if packed:
            nice.decode_batch_packed(self.packed if data is None else data, self.off if off is None else off, lens,
                                     self.w, self.h, out_channels, dec, status, flags=flags, host_len=host_len,
                                     packed_bytes=self.total if packed_bytes is None else packed_bytes)
        else:
            nice.decode_batch(self.strided, lens, self.w, self.h, out_channels, dec, status, flags=flags,
                              host_len=host_len)
        torch.cuda.synchronize()
        return dec, status.cpu().numpy()


@pytest.fixture(scope="module")
def rgba(nice, O):
    return Batch(nice, O, 6, 640, 360, 4)


@pytest.fixture(scope="module")
def rgb(nice, O):
    return Batch(nice, O, 5, 322, 201, 3)


@pytest.mark.parametrize("which", ["rgba", "rgb"])
def test_round_trip_in_place(nice, request, which):
    import torch
    b = request.getfixturevalue(which)
    assert int(b.status[0]) == 0
    assert torch.equal(b.plens, b.lens)
    lens = b.lens.cpu().numpy()
    off = b.off.cpu().numpy()
    assert off[0] == 0 and np.array_equal(np.diff(off), (lens + 15) // 16 * 16)
    blob = b.packed[:b.total].cpu().numpy()
    strided = b.strided.cpu().numpy()
    for f in range(b.n):
        s = blob[off[f]:off[f] + lens[f]].tobytes()
        assert s == strided[f, :lens[f]].tobytes(), f
        assert s == b.oracle[f], f
        assert not blob[off[f] + lens[f]:off[f + 1]].any(), f   # pads are zero
    oc = b.c
    for host_len in (None, lens.tolist()):
        dec, status = b.decode(nice, True, oc, nice.DEC_ALPHA_FILL_FF, host_len=host_len)
        assert (status == 0).all(), status
        d = dec.view(b.n, -1, oc)
        assert torch.equal(d[:, :, :3], b.rgb())
        if oc == 4:
            assert bool((d[:, :, 3] == 255).all())


@pytest.mark.parametrize("route", ["NICE_DEC_SLICE_BITS=1024", "NICE_DEC_NO_EVENTS=1", "NICE_DEC_SLOW_PARSE=1",
                                   "NICE_DEC_EV_CAP=4", "strict"])
def test_every_parse_route_reads_through_offset(nice, O, opts, request, route):
    import torch
    if route == "strict":
        b = request.getfixturevalue("rgb")
        for f in range(b.n):   # the reference decoder reads these streams to the end
            assert np.array_equal(O.decode(b.oracle[f])[0].reshape(-1), b.frames[f].reshape(-1)), f
        oc, flags = 3, nice.DEC_STRICT_REFERENCE
    else:
        b = request.getfixturevalue("rgba")
        name, value = route.split("=")
        opts.setenv(name, value)
        oc, flags = 4, nice.DEC_ALPHA_FILL_FF
    want, st0 = b.decode(nice, False, oc, flags)
    got, st1 = b.decode(nice, True, oc, flags)
    assert (st0 == 0).all() and (st1 == 0).all(), (st0, st1)
    assert torch.equal(got, want)
    assert torch.equal(got.view(b.n, -1, oc)[:, :, :3], b.rgb())


def test_subset_and_order(nice, rgba):
    import torch
    b = rgba
    pick = torch.tensor([4, 0, 4, 2], device="cuda")
    dec, status = b.decode(nice, True, 4, nice.DEC_ALPHA_FILL_FF, off=b.off[pick], lens=b.lens[pick],
                           packed_bytes=int(b.off[6]))
    assert (status == 0).all(), status
    assert torch.equal(dec.view(4, -1, 4)[:, :, :3], b.rgb()[pick])


def test_bad_offsets_fail_the_frame(nice, rgba):
    import torch
    b = rgba
    off = b.off[:b.n].clone()
    lens_h = b.lens.cpu().numpy()
    off_h = b.off.cpu().numpy()
    off[1] += 8                                       # not on a granule
    data = b.packed.clone()
    data[int(off_h[2]) + 7] ^= 1                      # frame 2: another width in its header
    packed_bytes = int(off_h[5] + lens_h[5]) - 1      # frame 5 ends one byte past the buffer
    assert off_h[4] + lens_h[4] <= packed_bytes and int(off[1]) + lens_h[1] <= packed_bytes
    dec, status = b.decode(nice, True, 4, nice.DEC_ALPHA_FILL_FF, off=off, packed_bytes=packed_bytes, data=data)
    assert status.tolist() == [0, E_ARG, E_ARG, 0, 0, E_ARG], status
    good = [0, 3, 4]
    assert torch.equal(dec.view(b.n, -1, 4)[good][:, :, :3], b.rgb()[good])
