#!/usr/bin/env python3
"""Timing of tiled images (include/nice.h, "tiled images") on one GPU, beside the
whole-frame codec on the same images in the same run:

* decode: decode_tiled against decode_batch of the one whole-frame stream, HIP
  events, alternated, median and spread;
* encode: encode_tiled (a blocking call: wall clock between device syncs)
  against encode_batch, and the share of it spent in the verify decode (the
  decoder's phase timers, nice_ctx_set_timing, in a run of their own);
* split and merge: (bytes read + bytes written) / time beside a torch copy_ of
  the same bytes;
* size: tiled bytes over the whole-frame stream, and the raw-tile count.

    python tools/bench_tiled.py [--sizes 3840x2160,16384x16384] [--tiles 512x512,1024x1024,1024x512]
                                [--runs 7] [--log FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "fast-losless-image-compression-format_amd"
N_PHASES, FIRST_DEC_PHASE = 16, 9   # include/nice.h: NICE_PHASES, NICE_PH_DEC_TABLES


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ts):
    s = sorted(ts)
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4),
            "runs": len(s)}


def pairs(text):
    return [tuple(int(v) for v in p.lower().split("x")) for p in text.split(",")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="3840x2160,16384x16384")
    ap.add_argument("--tiles", default="512x512,1024x1024,1024x512")
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
    report = {"device": torch.cuda.get_device_name(dev), "images": []}
    ok = True

    for W, H in pairs(args.sizes):
        px = bench.syn_frames(torch, 1, W, H, 1, dev)
        img = px.view(H, W, 4)
        stride = (nice.encode_bound(W, H) + 255) // 256 * 256
        stream = torch.empty((1, stride), dtype=torch.uint8, device=dev)
        slen = torch.zeros(1, dtype=torch.int64, device=dev)
        whole = torch.empty((1, W * H * 4), dtype=torch.uint8, device=dev)
        wstatus = torch.zeros(1, dtype=torch.int32, device=dev)

        def enc_whole():
            nice.encode_batch(px, W, H, 4, stream, slen, ctx=ctx)

        enc_whole()
        torch.cuda.synchronize()
        hl = slen.cpu().tolist()

        def dec_whole():
            nice.decode_batch(stream, slen, W, H, 4, whole, wstatus, host_len=hl, ctx=ctx)

        dec_whole()
        t_enc_whole = [wall_ms(torch, enc_whole) for _ in range(args.runs)]
        entry = {"image": f"{W}x{H} RGBA SYN-v1 seed 1", "whole_stream_bytes": hl[0],
                 "whole_encode": summary(t_enc_whole), "tiles": []}
        out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
        t_dec_whole = []
        for tw, th in pairs(args.tiles):
            timg = nice.encode_tiled(img, tile=(tw, th), ctx=ctx)   # warm: scratch sized
            t_enc = [wall_ms(torch, lambda: nice.encode_tiled(img, tile=(tw, th), ctx=ctx)) for _ in range(args.runs)]
            # the verify decode's share, from the decoder's phase timers
            L.nice_ctx_set_timing(ctx.ptr, 1)
            t_timed = wall_ms(torch, lambda: nice.encode_tiled(img, tile=(tw, th), ctx=ctx))
            ms = (ctypes.c_double * N_PHASES)()
            cnt = (ctypes.c_uint32 * N_PHASES)()
            L.nice_ctx_read_timing(ctx.ptr, ms, cnt)
            L.nice_ctx_set_timing(ctx.ptr, 0)
            verify_ms = sum(ms[FIRST_DEC_PHASE:])
            enc_ms = sum(ms[:FIRST_DEC_PHASE])

            def dec_tiled():
                nice.decode_tiled(timg, out=out, ctx=ctx)

            dec_tiled()
            t_dec = []
            for _ in range(args.runs):   # alternated with the whole-frame decode
                t_dec_whole.append(event_ms(torch, dec_whole))
                t_dec.append(event_ms(torch, dec_tiled))
            same = bool(torch.equal(out.view(-1, 4)[:, :3], px.view(-1, 4)[:, :3])) and int(wstatus[0]) == 0 and \
                bool(torch.equal(whole.view(-1, 4)[:, :3], px.view(-1, 4)[:, :3]))
            ok = ok and same
            # where the tiled decode's time goes: the decoder's phases, in a run of their own
            L.nice_ctx_set_timing(ctx.ptr, 1)
            t_dec_timed = wall_ms(torch, dec_tiled)
            L.nice_ctx_read_timing(ctx.ptr, ms, cnt)
            L.nice_ctx_set_timing(ctx.ptr, 0)
            L.nice_phase_name.restype = ctypes.c_char_p
            dec_phases = {L.nice_phase_name(i).decode(): round(ms[i], 3) for i in range(FIRST_DEC_PHASE, N_PHASES)}
            roi = (W // 2 - 256, H // 2 - 256, 512, 512)
            t_roi = [event_ms(torch, lambda: nice.decode_tiled(timg, roi=roi, ctx=ctx)) for _ in range(args.runs)]
            entry["tiles"].append({
                "tile": f"{tw}x{th}", "grid": f"{timg.nx}x{timg.ny}", "raw_tiles": int(timg.kind.sum()),
                "tiled_bytes": timg.nbytes, "size_ratio": round(timg.nbytes / hl[0], 4),
                "encode_tiled": summary(t_enc),
                "encode_tiled_timed_run": {"wall_ms": round(t_timed, 3), "encode_phases_ms": round(enc_ms, 3),
                                           "verify_decode_phases_ms": round(verify_ms, 3),
                                           "verify_share_of_wall": round(verify_ms / t_timed, 3)},
                "decode_tiled": summary(t_dec),
                "decode_tiled_timed_run": dict(dec_phases, wall_ms=round(t_dec_timed, 3)), "decode_roi_512x512": summary(t_roi), "round_trip_exact": same})
            del timg
        entry["whole_decode"] = summary(t_dec_whole)
        for t in entry["tiles"]:
            t["decode_speedup_vs_whole"] = round(entry["whole_decode"]["median_ms"] / t["decode_tiled"]["median_ms"], 2)
            t["encode_slowdown_vs_whole"] = round(t["encode_tiled"]["median_ms"] / entry["whole_encode"]["median_ms"], 2)

        # ---- split and merge beside a copy of the same bytes (the last, largest image is the one DESIGN.md quotes)
        tw, th = 1024, 512
        nx, ny = nice.tile_grid(W, H, tw, th)
        n, tstride = nx * ny, tw * th * 4
        tiles = torch.empty(n * tstride, dtype=torch.uint8, device=dev)
        idx = torch.arange(n, dtype=torch.int32, device=dev)
        p = ctypes.c_void_p

        def split():
            assert L.nice_tiles_split_dev(ctx.ptr, p(torch.cuda.current_stream().cuda_stream), p(px.data_ptr()), W * 4,
                                          W, H, 4, tw, th, p(tiles.data_ptr()), tstride) == 0

        def merge():
            assert L.nice_tiles_merge_dev(ctx.ptr, p(torch.cuda.current_stream().cuda_stream), p(tiles.data_ptr()),
                                          tstride, p(idx.data_ptr()), n, 4, W, H, tw, th, 0, 0, W, H, 4, 0,
                                          p(out.data_ptr()), W * 4) == 0

        def copy():
            whole.view(-1).copy_(px.view(-1))

        for fn in (split, merge, copy):
            fn()
        ts, tm, tc = [], [], []
        for _ in range(args.runs):
            tc.append(event_ms(torch, copy))
            ts.append(event_ms(torch, split))
            tm.append(event_ms(torch, merge))
        ok = ok and bool(torch.equal(out.view(-1), px.view(-1)))
        img_bytes = W * H * 4

        def gbs(nbytes, t):
            return round(nbytes / (statistics.median(t) * 1e-3) / 1e9, 1)

        entry["copies_1024x512"] = {
            "copy": dict(summary(tc), gb_s=gbs(2 * img_bytes, tc)),
            "split": dict(summary(ts), gb_s=gbs(img_bytes + n * tstride, ts)),
            "merge": dict(summary(tm), gb_s=gbs(2 * img_bytes, tm)),
            "split_vs_copy": round(gbs(img_bytes + n * tstride, ts) / gbs(2 * img_bytes, tc), 3),
            "merge_vs_copy": round(gbs(2 * img_bytes, tm) / gbs(2 * img_bytes, tc), 3)}
        report["images"].append(entry)
        del px, img, stream, whole, out, tiles
        torch.cuda.empty_cache()

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
