"""enc_pack's over-cap path (hfe.rs:110-113, bitwriter.rs:55-73).

A packer group (4 tiles, 4096 pixels) collects its codes in an LDS buffer of
32 bits per pixel.  A group that goes over it -- only possible after its first
tiles have already been OR-ed into the buffer -- is counted and OR-ed into the
output directly instead, and the next group on the block must clear the whole
buffer.  The test hook pack_cap_bpp=b lowers the buffer to b bits per pixel so ordinary
frames reach that path (mid-group, after tiles were written); a frame with one
row of noise in a smooth image reaches it at the real cap.  Every stream must
equal the oracle's byte for byte.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE, GROUP = 1024, 4096   # ENC_TILE; PACK_SUB tiles: one packer group
# (start, L): the coded pixel `start` and L repeats of it, over linear pixel
# ranges (as tests/test_classify_stages.py): runs of one to five base-8 digits,
# from a wave's last lane, across a wave boundary, across in-tile offset 511 |
# 512, to a tile's last pixel, across tile ends and across whole groups
RARE_SPANS = ((1124, 5), (1224, 10), (1324, 70), (2098, 600), (3199, 4), (3322, 7), (4601, 20), (6120, 23),
              (7154, 30), (12788, 200), (13412, 66), (13612, 130), (40967, 5000))
# shape -> (noise rows, groups over 32 bits per pixel, last tile's pixels, longest pixel's bits at seed 1)
RARE_SHAPES = {(2051, 66): ((6, 7, 8, 9, 30), 1, 198, 65), (4099, 33): ((3, 4, 20), 2, 99, 62)}


@functools.lru_cache(maxsize=None)
def _rare_input(w, h, c, seed=1):
    """(pixels, the oracle's stream) of one small frame that reaches every rare
    stage of the pack kernels at once: gen_rgb_field with noise rows (pixels and
    whole groups over 32 bits) and RARE_SPANS plus a run to the last pixel, the
    pixels either side of a span differing from it.  The properties the cases
    below rely on are asserted from the oracle, so a generator change fails
    here instead of testing nothing."""
    from conftest import oracle_mod
    O = oracle_mod()
    rows, n_over, last_px, longest = RARE_SHAPES[(w, h)]
    n = w * h
    px = O.gen_rgb_field(w, h, c, seed, list(rows)).reshape(n, c).copy()
    for k, (s, L) in enumerate(RARE_SPANS + ((n - 12, 11),)):
        colour = np.array([17 + 5 * k, 201 - 3 * k, 90 + k, 255][:c], dtype=np.uint8)
        px[s:s + L + 1] = colour
        for j in (s - 1, s + L + 1):
            if j < n:
                px[j] = colour
                px[j, 0] ^= 0x80
    px = px.reshape(-1)
    stream, st = O.encode(px, w, h, c, with_stats=True)
    s2, bits = O.encode_bitpos(px, w, h, c)
    assert s2 == stream
    tiles = (n + TILE - 1) // TILE
    assert tiles == 133 and n - (tiles - 1) * TILE == last_px   # 33 full groups, one of a single partial tile
    assert n % 4 == (2 if w == 2051 else 3)                     # the scalar record loads
    assert st.max_emitted_aob == 12                             # the one-pass packer, not the long path
    # a pixel's codes start at its entry and end where the next coded pixel's start (run members: 2^64 - 1)
    nxt = np.minimum.accumulate(bits[::-1])[::-1]
    coded = np.flatnonzero(bits[:n] != np.uint64(2 ** 64 - 1))
    px_bits = (nxt[coded + 1] - bits[coded]).astype(np.int64)
    runs = np.diff(np.append(coded, n)) - 1
    group_bits = np.diff(np.append(nxt[np.arange(0, n, GROUP)], bits[n])).astype(np.int64)
    assert len(group_bits) == 34
    assert int((group_bits > 32 * GROUP).sum()) == n_over       # over the real cap
    assert int((group_bits > 8 * GROUP).sum()) == 31            # over a cap of 8 bits per pixel
    assert 0 < int((group_bits > 11 * GROUP).sum()) < 34        # both kinds at a cap of 11
    assert int((px_bits > 32).sum()) > 10000                    # enc_pack's entry-by-entry tier
    assert px_bits.max() >= 62 and (seed != 1 or px_bits.max() == longest)
    assert int((runs > 64).sum()) == 6 and runs.max() == 5000   # extra run digits, up to five digits
    assert all(int(st.hist[256 + 5 + d]) for d in range(8))     # BIN_PREFIX + P_RUN1 + d (csrc/nice_format.h)
    return px, stream


def _first_diff(got, want):
    if got != want:
        d = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        pytest.fail(f"first differing byte {d} of {len(want)} (got {len(got)})")


@pytest.fixture
def cap_hook(nice):
    """Sets the default context's packer cap (bits per pixel); reset after."""
    from conftest import set_hooks
    ctx = nice._ctx(0)
    yield lambda b: set_hooks(nice, ctx, pack_cap_bpp=b)
    set_hooks(nice, ctx)


@pytest.mark.parametrize("cap", [4, 8, 12])
def test_pack_cap_single_frames(nice, O, cap, cap_hook):
    cap_hook(cap)
    for w, h, c, seed in [(1920, 1080, 4, 3), (4096, 64, 4, 5), (1000, 333, 3, 2)]:
        px = O.gen_syn_v1(w, h, c, seed)
        want = O.encode(px, w, h, c)
        got = nice.encode_bytes(px, w, h, c)
        assert got == want, (w, h, c, cap)


def test_pack_cap_batch(nice, O, cap_hook):
    """A batch: blocks move between frames and reuse their LDS buffer across
    over-cap and ordinary groups."""
    import torch
    cap_hook(11)   # SYN-v1 averages ~10.7 bits/px: both kinds of group
    w, h, c, n = 1280, 720, 4, 6
    frames = np.stack([O.gen_syn_v1(w, h, c, s) for s in range(1, n + 1)])
    px = torch.from_numpy(frames).cuda()
    bound = (nice.encode_bound(w, h) + 255) // 256 * 256
    out = torch.zeros((n, bound), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    nice.encode_batch(px, w, h, c, out, lens)
    torch.cuda.synchronize()
    L = lens.cpu().numpy()
    host = out.cpu().numpy()
    for i in range(n):
        want = O.encode(frames[i], w, h, c)
        assert bytes(host[i, :L[i]]) == want, i


def test_pack_cap_bands(nice, O):
    import importlib
    import torch
    from conftest import PKG_NAME, set_hooks
    S = importlib.import_module(PKG_NAME + ".sharded")
    w, h, c, R = 2048, 512, 4, 3
    px = O.gen_syn_v1(w, h, c, 4)
    want = O.encode(px, w, h, c)
    backends = []
    for _ in range(R):
        be = S.HipBands(0)
        be.ctx = nice._Ctx(0)
        set_hooks(nice, be.ctx, pack_cap_bpp=8)
        backends.append(be)
    got = S.encode_bands(torch.from_numpy(px).cuda(), w, h, c, R, backends=backends).cpu().numpy().tobytes()
    assert got == want


def test_pack_noise_row_real_cap(nice, O):
    """Rows of uniform noise in a 4096-wide frame of RGB-mode pixels with
    geometric residuals (oracle gen_rgb_field): each noise row is one packer
    group whose residuals take the rare 15-17 bit codes of stream 0, about 50
    bits per pixel, so the group goes over the real cap after its first tiles;
    the groups after it reuse the buffer."""
    w, h, c = 4096, 1024, 4
    px = O.gen_rgb_field(w, h, c, 1, [300, 301, 400])
    want, st = O.encode(px, w, h, c, with_stats=True)
    assert st.max_emitted_aob <= 25   # not a long-code frame: the one-pass packer runs
    aob = np.array(st.aob[0:256])
    rare = aob[np.array(st.hist[0:256]) > 0].max()
    assert 3 * rare > 40, rare        # a noise pixel: prefix + three rare residuals
    got = nice.encode_bytes(px, w, h, c)
    assert got == want


def test_pack_rare_path_mixed(nice, O):
    """Waves whose pixels mix >32-bit codes (noise in a frame of RGB-mode
    pixels with geometric residuals) with runs longer than 64 pixels (extra
    run digits, code.rs:391-406): the packer's entry-by-entry path, next to
    ordinary waves; the stream must equal the oracle's."""
    w, h, c = 2048, 256, 4
    px = O.gen_rgb_field(w, h, c, 3, [40, 41, 200]).reshape(h, w, c)
    for y in (40, 41, 200):          # noise rows cut by runs of 65..300 pixels
        x = 17
        while x < w - 400:
            n = 65 + (x * 7) % 236
            px[y, x:x + n, :3] = px[y, x, :3]
            x += n + 50
    px[120, 100:1900, :3] = (5, 6, 7)   # one long run in the smooth field
    px = px.reshape(-1)
    want, st = O.encode(px, w, h, c, with_stats=True)
    assert st.max_emitted_aob <= 25
    got = nice.encode_bytes(px, w, h, c)
    if got != want:
        d = next(i for i in range(min(len(got), len(want))) if got[i] != want[i])
        pytest.fail(f"first differing byte {d} of {len(want)} (got {len(got)})")


@pytest.mark.parametrize("cap", [None, 8], ids=["real-cap", "cap8"])
@pytest.mark.parametrize("c", [4, 3], ids=["rgba", "rgb"])
@pytest.mark.parametrize("shape", sorted(RARE_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_rare_stages_single_frames(nice, shape, c, cap, cap_hook):
    """The rare-stage frame at the real cap (one or two groups to
    enc_pack_over, the rest through enc_pack's entry-by-entry tier and extra
    run digits) and at a cap of 8 bits per pixel (enc_pack_over on almost every
    group, the one-tile group and the partial tile included)."""
    w, h = shape
    px, want = _rare_input(w, h, c)
    if cap is not None:
        cap_hook(cap)
    _first_diff(nice.encode_bytes(px, w, h, c), want)


def test_pack_rare_stages_batch(nice, cap_hook):
    """Three rare-stage frames as one batch at a cap of 11: blocks change
    frames and reload their tables between over-cap and ordinary groups."""
    import torch
    cap_hook(11)
    w, h, c = 2051, 66, 4
    inputs = [_rare_input(w, h, c, seed) for seed in (1, 2, 3)]
    n = len(inputs)
    px = torch.from_numpy(np.stack([p for p, _ in inputs])).cuda()
    bound = (nice.encode_bound(w, h) + 255) // 256 * 256
    out = torch.zeros((n, bound), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    nice.encode_batch(px, w, h, c, out, lens)
    torch.cuda.synchronize()
    L = lens.cpu().numpy()
    host = out.cpu().numpy()
    for i in range(n):
        _first_diff(bytes(host[i, :L[i]]), inputs[i][1])


def test_pack_rare_stages_bands(nice):
    """The rare-stage frame as three bands at a cap of 8 on each backend (the
    coded flags come from the records there, not from the classify's mask)."""
    import importlib
    import torch
    from conftest import PKG_NAME, set_hooks
    S = importlib.import_module(PKG_NAME + ".sharded")
    w, h, c, R = 4099, 33, 4, 3
    px, want = _rare_input(w, h, c)
    backends = []
    for _ in range(R):
        be = S.HipBands(0)
        be.ctx = nice._Ctx(0)
        set_hooks(nice, be.ctx, pack_cap_bpp=8)
        backends.append(be)
    got = S.encode_bands(torch.from_numpy(px).cuda(), w, h, c, R, backends=backends).cpu().numpy().tobytes()
    _first_diff(got, want)
