"""The raster store the five multi-wave row kernels share (rows_store_raster,
csrc/nice_rows.hip), through each of them: dec_rows, dec_rows_flow with one and
two row groups, dec_rows_split and dec_rows_wide, at widths that take its
16-byte paths for both output formats (1600, 8208: W % 16 == 0), for RGBA only
(1604, 8212: W % 4 == 0) and its scalar paths (1603, 8211), RGB and RGBA
streams into 3 and 4 output channels.  Each case asserts status 0, the route
the library reports (so an option that stops forcing its kernel fails here
instead of testing another one), the input's pixels and, with four channels,
the alpha fill."""
import functools

import numpy as np
import pytest

import plan_driver
from test_width_sweep import H, _frame

pytestmark = pytest.mark.gpu

NARROW, WIDE = (1600, 1603, 1604), (8208, 8211, 8212)
# id -> (kernel, test options, widths)
ROUTES = {
    "rows": ("dec_rows", {"NICE_DEC_FLOW": 0, "NICE_DEC_SPLIT": 0}, NARROW),
    "flow1": ("dec_rows_flow", {"NICE_DEC_FLOW": 1}, NARROW),
    "flow2": ("dec_rows_flow", {"NICE_DEC_FLOW": 2}, NARROW),
    "split2": ("dec_rows_split", {"NICE_DEC_SPLIT": 2}, NARROW),
    "wide": ("dec_rows_wide", {"NICE_DEC_SPLIT": 0}, WIDE),
    "split": ("dec_rows_split", {}, WIDE),
}
CASES = [(r, w) for r, (_, _, widths) in ROUTES.items() for w in widths]


@functools.lru_cache(maxsize=None)
def _stream(W, C):
    """(RGB bytes of the frame, its stream as a padded cuda row, length), once
    per shape; the oracle's tolerant decode gives the frame back."""
    import torch
    from conftest import oracle_mod
    O = oracle_mod()
    px = _frame(O, W, C, W * 7 + C)
    s = O.encode(px, W, H, C)
    rgb = px.reshape(-1, C)[:, :3].copy()
    ref, _ = O.decode(s[:12] + bytes([3]) + s[13:], O.DEC_TOLERANT)
    assert np.array_equal(np.asarray(ref).reshape(-1, 3), rgb), (W, C)
    sb = torch.zeros((1, (len(s) + 255) // 256 * 256), dtype=torch.uint8)
    sb[0, :len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
    return rgb, sb.cuda(), torch.tensor([len(s)], dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("route,W", CASES, ids=[f"{r}-{w}" for r, w in CASES])
def test_rows_store(nice, opts, route, W):
    import torch
    kernel, options, _ = ROUTES[route]
    for name, value in options.items():
        opts.setenv(name, value)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    want = plan_driver.plan(W, H, 1, cus, **{k[len("NICE_DEC_"):].lower(): v for k, v in options.items()})
    assert want["route"] == kernel
    ctx = nice.Context(0)
    for C in (3, 4):
        rgb, sb, lens = _stream(W, C)
        for OC in (3, 4):
            dec = torch.zeros((1, W * H * OC), dtype=torch.uint8, device="cuda")
            status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            nice.decode_batch(sb, lens, W, H, OC, dec, status,
                              flags=nice.DEC_ALPHA_FILL_FF | nice.DEC_TOLERANT_HEADER, ctx=ctx)
            torch.cuda.synchronize()
            assert int(status[0]) == 0, (C, OC)
            assert plan_driver.last_route(nice, ctx) == (kernel, want["fallback"]), (C, OC)
            got = dec[0].view(-1, OC).cpu().numpy()
            assert np.array_equal(got[:, :3], rgb), (C, OC)
            if OC == 4:
                assert (got[:, 3] == 255).all(), C
