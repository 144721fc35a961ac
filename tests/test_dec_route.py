"""The row kernel a decode really launches is the one the planner names: one
SYN-v1 RGBA frame of 8 rows per width, no options set -- dec_reconstruct below
64 columns, the dataflow kernel up to 8192 (two row groups, then one), the
strip split above, with dec_rows, dec_rows_wide and dec_reconstruct as the
redo launches.  The route and fallback the library reports
(nice_test_last_dec_route) must be the plan of tools/dec_plan_check.cpp for the
same shape and the device's CU count, and the pixels exact."""
import numpy as np
import pytest

import plan_driver

pytestmark = pytest.mark.gpu

H = 8


@pytest.mark.parametrize("W", [32, 64, 1920, 5000, 8208, 20000])
def test_route_matches_plan(nice, O, opts, W):
    import torch
    px = O.gen_syn_v1(W, H, 4, W)
    s = O.encode(px, W, H, 4)
    sb = torch.zeros((1, (len(s) + 255) // 256 * 256), dtype=torch.uint8)
    sb[0, :len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
    sb = sb.cuda()
    lens = torch.tensor([len(s)], dtype=torch.int64, device="cuda")
    dec = torch.zeros((1, W * H * 4), dtype=torch.uint8, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ctx = nice.Context(0)
    # tolerant header: small frames' tables are outside the reference decoder's domain
    nice.decode_batch(sb, lens, W, H, 4, dec, status, flags=nice.DEC_ALPHA_FILL_FF | nice.DEC_TOLERANT_HEADER, ctx=ctx)
    torch.cuda.synchronize()
    assert int(status[0]) == 0
    got = dec[0].view(-1, 4).cpu().numpy()
    assert np.array_equal(got[:, :3], px.reshape(-1, 4)[:, :3])   # the stream carries no alpha
    assert (got[:, 3] == 255).all()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    want = plan_driver.plan(W, H, 1, cus)
    assert plan_driver.last_route(nice, ctx) == (want["route"], want["fallback"])


def test_too_wide_rows_are_refused(nice, opts):
    """From 39345 columns no row kernel fits a row's records beside its static
    LDS: the call returns NICE_E_ARG before it launches anything, and the
    narrower neighbour still plans the strip split."""
    import torch
    W = 39345
    sb = torch.zeros((1, 1024), dtype=torch.uint8, device="cuda")
    lens = torch.tensor([1024], dtype=torch.int64, device="cuda")
    dec = torch.zeros((1, W * H * 4), dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx = nice.Context(0)
    with pytest.raises(nice.NiceError) as e:
        nice.decode_batch(sb, lens, W, H, 4, dec, status, ctx=ctx)
    assert e.value.code == -1
    assert plan_driver.last_route(nice, ctx) == ("none", "none")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert plan_driver.plan(W - 1, H, 1, cus)["route"] == "dec_rows_split"
