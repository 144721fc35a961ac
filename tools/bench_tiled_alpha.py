#!/usr/bin/env python3
"""Timing of the alpha batch of tiled images (include/nice.h, "tiled images:
alpha") on one GPU, beside the alpha-less calls on the same image in the same
run.  HIP events (wall clock between device syncs for the blocking encodes),
alternated runs, median and spread.  The image is RGBA SYN-v1, once opaque and
once with a soft-mask alpha (a feathered disc).

* range pass: nice_tiles_alpha_range_dev against nice_tiles_split_dev of the
  same image (the same bytes read, almost nothing written);
* opaque: encode_tiled(alpha=True) against encode_tiled(), and a 4-channel
  decode_tiled with and without the alpha batch; the alpha merge of constant
  tiles alone, (bytes read + written) / time beside a torch copy_;
* soft mask: the alpha encode and the alpha decode alone, each also split by
  the codec's phase timers in a run of its own, the kinds, and the alpha bytes
  over the raw plane's.

    python tools/bench_tiled_alpha.py [--size 16384x16384] [--tile 1024x512] [--runs 7] [--log FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import dataclasses
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = "fast-losless-image-compression-format_amd"

from bench_tiled import FIRST_DEC_PHASE, N_PHASES, event_ms, summary, wall_ms  # noqa: E402


def soft_mask(torch, w, h, dev):
    """Alpha of a feathered disc: 255 inside, 0 outside, a ramp of min(w, h) / 32 pixels between."""
    r, f = 0.36 * min(w, h), min(w, h) / 32
    y = torch.arange(h, device=dev, dtype=torch.float32)[:, None] - h / 2
    x = torch.arange(w, device=dev, dtype=torch.float32)[None, :] - w / 2
    return ((r - torch.sqrt(x * x + y * y)) * (255 / f)).clamp_(0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="16384x16384")
    ap.add_argument("--tile", default="1024x512")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--log", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch
    import bench
    nice = importlib.import_module(PKG)
    L = nice.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = nice.Context(0)
    W, H = (int(v) for v in args.size.lower().split("x"))
    tw, th = (int(v) for v in args.tile.lower().split("x"))
    nx, ny = nice.tile_grid(W, H, tw, th)
    n = nx * ny
    p = ctypes.c_void_p
    img = bench.syn_frames(torch, 1, W, H, 1, dev).view(H, W, 4)
    img_bytes = W * H * 4
    report = {"device": torch.cuda.get_device_name(dev), "image": f"{W}x{H} RGBA SYN-v1 seed 1", "tile": f"{tw}x{th}",
              "grid": f"{nx}x{ny}"}
    ok = True

    def gbs(nbytes, ts):
        return round(nbytes / (statistics.median(ts) * 1e-3) / 1e9, 1)

    def cur():
        return p(torch.cuda.current_stream().cuda_stream)

    # ---- opaque ------------------------------------------------------------------
    img[:, :, 3] = 255
    tiles = torch.empty(n * tw * th * 4, dtype=torch.uint8, device=dev)
    lo = torch.empty(n, dtype=torch.int32, device=dev)
    hi = torch.empty(n, dtype=torch.int32, device=dev)
    other = torch.empty_like(img)

    def split():
        assert L.nice_tiles_split_dev(ctx.ptr, cur(), p(img.data_ptr()), W * 4, W, H, 4, tw, th, p(tiles.data_ptr()),
                                      tw * th * 4) == 0

    def arange():
        assert L.nice_tiles_alpha_range_dev(ctx.ptr, cur(), p(img.data_ptr()), W * 4, W, H, tw, th, p(lo.data_ptr()),
                                            p(hi.data_ptr())) == 0

    def copy():
        other.view(-1).copy_(img.view(-1))

    for fn in (split, arange, copy):
        fn()
    ts, tr, tc = [], [], []
    for _ in range(args.runs):
        tc.append(event_ms(torch, copy))
        ts.append(event_ms(torch, split))
        tr.append(event_ms(torch, arange))
    ok = ok and bool((lo == 255).all()) and bool((hi == 255).all())
    report["range_pass"] = {
        "range": dict(summary(tr), gb_s_read=gbs(img_bytes, tr)),
        "split": dict(summary(ts), gb_s_read_and_written=gbs(img_bytes + n * tw * th * 4, ts)),
        "copy": dict(summary(tc), gb_s_read_and_written=gbs(2 * img_bytes, tc)),
        "range_over_split": round(statistics.median(tr) / statistics.median(ts), 3),
        "split_spread_ms": round(max(ts) - min(ts), 4),
        "range_within_split_plus_spread": statistics.median(tr) <= statistics.median(ts) + (max(ts) - min(ts))}
    del tiles
    torch.cuda.empty_cache()

    plain = nice.encode_tiled(img, tile=(tw, th), ctx=ctx)                 # warm: scratch sized
    both = nice.encode_tiled(img, tile=(tw, th), ctx=ctx, alpha=True)
    te_plain, te_alpha = [], []
    for _ in range(args.runs):
        te_plain.append(wall_ms(torch, lambda: nice.encode_tiled(img, tile=(tw, th), ctx=ctx)))
        te_alpha.append(wall_ms(torch, lambda: nice.encode_tiled(img, tile=(tw, th), ctx=ctx, alpha=True)))
    out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    for t in (plain, both):
        nice.decode_tiled(t, out=out, ctx=ctx)
    td_plain, td_alpha = [], []
    for _ in range(args.runs):
        td_plain.append(event_ms(torch, lambda: nice.decode_tiled(plain, out=out, ctx=ctx)))
        td_alpha.append(event_ms(torch, lambda: nice.decode_tiled(both, out=out, ctx=ctx)))
    ok = ok and bool(torch.equal(out, img)) and bool((both.alpha.kind == 2).all()) and both.alpha.nbytes == 0

    def alpha_decode(t):
        a = t.alpha
        tabs = [a.off, a.stream_len, a.kind, a.value]
        st = torch.empty(n, dtype=torch.int32, device=dev)

        def run():
            assert L.nice_decode_tiled_alpha_dev(ctx.ptr, cur(), p(a.packed.data_ptr() if a.nbytes else None), a.nbytes,
                                                 *[p(v.data_ptr()) for v in tabs], W, H, tw, th, 0, 0, W, H,
                                                 p(out.data_ptr()), W * 4, p(st.data_ptr())) == 0
        return run, st

    merge_const, _ = alpha_decode(both)
    merge_const()
    tm, tc = [], []
    for _ in range(args.runs):
        tc.append(event_ms(torch, copy))
        tm.append(event_ms(torch, merge_const))
    report["opaque"] = {
        "encode_tiled": summary(te_plain), "encode_tiled_alpha": summary(te_alpha),
        "encode_alpha_over_plain": round(statistics.median(te_alpha) / statistics.median(te_plain), 3),
        "decode_tiled_4ch": summary(td_plain), "decode_tiled_4ch_alpha": summary(td_alpha),
        "decode_alpha_over_plain": round(statistics.median(td_alpha) / statistics.median(td_plain), 3),
        "alpha_merge_constant_tiles": dict(summary(tm), gb_s_read_and_written=gbs(2 * img_bytes, tm)),
        "copy": dict(summary(tc), gb_s_read_and_written=gbs(2 * img_bytes, tc)),
        "alpha_tiles": {"coded": 0, "raw": 0, "constant": n}, "alpha_bytes": 0}
    del plain, both
    torch.cuda.empty_cache()

    # ---- soft mask ---------------------------------------------------------------
    img[:, :, 3] = soft_mask(torch, W, H, dev)
    pitch = W * 4

    def alpha_encode():
        return nice._encode_tiled_alpha(torch, img, pitch, tw, th, n, None, ctx)

    colour = nice.encode_tiled(img, tile=(tw, th), ctx=ctx)
    timg = dataclasses.replace(colour, alpha=alpha_encode())
    te = [wall_ms(torch, alpha_encode) for _ in range(args.runs)]
    nice.decode_tiled(timg, out=out, ctx=ctx)
    ok = ok and bool(torch.equal(out, img))
    dec_alpha, st = alpha_decode(timg)
    dec_alpha()
    td, tc = [], []
    for _ in range(args.runs):
        tc.append(event_ms(torch, copy))
        td.append(event_ms(torch, dec_alpha))
    ok = ok and bool((st == 0).all()) and bool(torch.equal(out, img))
    k = timg.alpha.kind
    plane = n * tw * th

    def timed(fn):
        """One run with the codec's phase timers: wall clock, encoder phases, decoder phases (ms)."""
        L.nice_phase_name.restype = ctypes.c_char_p
        L.nice_ctx_set_timing(ctx.ptr, 1)
        wall = wall_ms(torch, fn)
        ms = (ctypes.c_double * N_PHASES)()
        cnt = (ctypes.c_uint32 * N_PHASES)()
        L.nice_ctx_read_timing(ctx.ptr, ms, cnt)
        L.nice_ctx_set_timing(ctx.ptr, 0)
        dec = {L.nice_phase_name(i).decode(): round(ms[i], 3) for i in range(FIRST_DEC_PHASE, N_PHASES)}
        # outside the phases: the range pass and its wait, gather, compare, store, pack; upload, scatter, merge
        return {"wall_ms": round(wall, 3), "encode_phases_ms": round(sum(ms[:FIRST_DEC_PHASE]), 3),
                "decode_phases_ms": round(sum(ms[FIRST_DEC_PHASE:]), 3), "decode_phases": dec,
                "outside_the_phases_ms": round(wall - sum(ms), 3)}

    report["soft_mask"] = {
        "alpha": "feathered disc, radius 0.36 min(w, h), ramp min(w, h) / 32",
        "alpha_encode": summary(te), "alpha_encode_timed_run": timed(alpha_encode),
        "alpha_decode": summary(td), "alpha_decode_timed_run": timed(dec_alpha),
        "copy": dict(summary(tc), gb_s_read_and_written=gbs(2 * img_bytes, tc)),
        "alpha_tiles": {"coded": int((k == 0).sum()), "raw": int((k == 1).sum()), "constant": int((k == 2).sum())},
        "alpha_bytes": timg.alpha.nbytes, "raw_plane_bytes": plane,
        "alpha_bytes_over_plane": round(timg.alpha.nbytes / plane, 5),
        "alpha_bytes_over_colour_bytes": round(timg.alpha.nbytes / timg.nbytes, 5)}
    report["all_round_trips_exact"] = ok
    text = json.dumps(report, indent=1)
    print(text)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)) or ".", exist_ok=True)
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
