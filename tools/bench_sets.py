#!/usr/bin/env python3
"""Timing of image sets (include/nice.h, "image sets") on one GPU.  The workload
is K RGBA SYN-v1 images generated on the device, widths and heights drawn from
a fixed-seed list between 256 and 1536.

1. the bar: encode_set / decode_set of all K images against the only other
   means to the same end, a loop of encode_tiled / decode_tiled over the same
   images at the same tile size, alternated in one run (all four calls block:
   wall clock between device syncs);
2. the copies: a one-image set of 8192 x 8192 RGBA at 1024 x 512, set_split and
   set_merge beside tiles_split and tiles_merge on the same image and a device
   copy of the same bytes (HIP events, alternated);
3. the default tile: the set at 256 x 256, 512 x 512 and 1024 x 512: encode and
   decode time, container bytes, raw tiles, the decoder's phase timers;
4. the crop batch: K windows of 224 x 224, one per image at a fixed-seed
   position, into one [K, 224, 224, 4] tensor, against the full decode_set.

Every figure is a median of --runs with min, max and spread (max - min).

    python tools/bench_sets.py [--images 256] [--runs 7] [--tile 512x512] [--log profiles/sets_bench.json]
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "fast-losless-image-compression-format_amd"
N_PHASES, FIRST_DEC_PHASE = 16, 9   # include/nice.h: NICE_PHASES, NICE_PH_DEC_TABLES
SWEEP = [(256, 256), (512, 512), (1024, 512)]


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
            "spread_ms": round(s[-1] - s[0], 4), "runs": len(s)}


def wins(a, b):
    """a beats b by more than the noise: a's median plus its spread below b's median minus its spread."""
    return a["median_ms"] + a["spread_ms"] < b["median_ms"] - b["spread_ms"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--tile", default=None, help="tile of parts 1 and 4 (default: DEFAULT_SET_TILE)")
    ap.add_argument("--skip-copies", action="store_true", help="leave out part 2 (8192 x 8192)")
    ap.add_argument("--log", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch
    import bench
    nice = importlib.import_module(PKG)
    L = nice.lib()
    L.nice_phase_name.restype = ctypes.c_char_p
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = nice.Context(0)
    K, runs = args.images, args.runs
    tile = nice.DEFAULT_SET_TILE if args.tile is None else tuple(int(v) for v in args.tile.lower().split("x"))
    rng = np.random.default_rng(20)
    sizes = rng.integers(256, 1537, (K, 2)).tolist()
    imgs = [bench.syn_frames(torch, 1, w, h, 1 + i, dev).view(h, w, 4) for i, (w, h) in enumerate(sizes)]
    outs = [torch.empty_like(im) for im in imgs]
    pixels = sum(w * h for w, h in sizes)
    report = {"device": torch.cuda.get_device_name(dev), "images": K, "pixels": pixels,
              "sizes": "RGBA SYN-v1 seeds 1.., widths and heights numpy default_rng(20).integers(256, 1537)"}
    ok = True

    def exact():
        return all(bool(torch.equal(o[:, :, :3], im[:, :, :3])) for o, im in zip(outs, imgs))

    def phases(fn):
        L.nice_ctx_set_timing(ctx.ptr, 1)
        t = wall_ms(torch, fn)
        ms, cnt = (ctypes.c_double * N_PHASES)(), (ctypes.c_uint32 * N_PHASES)()
        L.nice_ctx_read_timing(ctx.ptr, ms, cnt)
        L.nice_ctx_set_timing(ctx.ptr, 0)
        d = {L.nice_phase_name(i).decode(): round(ms[i], 3) for i in range(FIRST_DEC_PHASE, N_PHASES)}
        d["launches_of_dec_tables"] = cnt[FIRST_DEC_PHASE]
        d["wall_ms"] = round(t, 3)
        return d

    # ---- 1. the set against the loop, at one tile size
    iset = nice.encode_set(imgs, tile=tile, ctx=ctx)                       # warm: scratch sized
    timgs = [nice.encode_tiled(im, tile=tile, ctx=ctx) for im in imgs]
    t = {k: [] for k in ("encode_set", "encode_loop", "decode_set", "decode_loop")}
    for _ in range(runs):
        t["encode_set"].append(wall_ms(torch, lambda: nice.encode_set(imgs, tile=tile, ctx=ctx)))
        t["encode_loop"].append(wall_ms(torch, lambda: [nice.encode_tiled(im, tile=tile, ctx=ctx) for im in imgs]))
        t["decode_set"].append(wall_ms(torch, lambda: nice.decode_set(iset, out=outs, ctx=ctx)))
        ok = ok and exact()
        for o in outs:
            o.zero_()
        t["decode_loop"].append(wall_ms(torch, lambda: [nice.decode_tiled(ti, out=o, ctx=ctx)
                                                        for ti, o in zip(timgs, outs)]))
        ok = ok and exact()
    s = {k: summary(v) for k, v in t.items()}
    same = all(bool(torch.equal(ti.packed, iset.packed[int(iset.off[a]):int(iset.off[b])]))
               for ti, a, b in zip(timgs, iset.first[:-1], iset.first[1:]))
    ok = ok and same
    report["bar"] = dict(s, tile=f"{tile[0]}x{tile[1]}", tiles=iset.first[-1], raw_tiles=int(iset.kind.sum()),
                         set_equals_concatenated_tiled_images=same,
                         decode_set_wins=wins(s["decode_set"], s["decode_loop"]),
                         encode_set_wins=wins(s["encode_set"], s["encode_loop"]),
                         decode_speedup=round(s["decode_loop"]["median_ms"] / s["decode_set"]["median_ms"], 2),
                         encode_speedup=round(s["encode_loop"]["median_ms"] / s["encode_set"]["median_ms"], 2),
                         decode_set_gpix_s=round(pixels / s["decode_set"]["median_ms"] / 1e6, 2),
                         encode_set_gpix_s=round(pixels / s["encode_set"]["median_ms"] / 1e6, 2),
                         decode_set_phases=phases(lambda: nice.decode_set(iset, out=outs, ctx=ctx)))
    del timgs

    # ---- 4. the crop batch
    cw = 224
    crops = [(i, int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - cw + 1)), cw, cw)
             for i, (w, h) in enumerate(sizes)]
    batch = torch.empty((K, cw, cw, 4), dtype=torch.uint8, device=dev)
    nice.decode_set(iset, windows=crops, out=batch, ctx=ctx)
    L.nice_test_last_set.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    nc, nr = ctypes.c_uint32(), ctypes.c_uint32()
    L.nice_test_last_set(ctx.ptr, ctypes.byref(nc), ctypes.byref(nr))
    ok = ok and all(bool(torch.equal(batch[j, :, :, :3], imgs[i][y:y + cw, x:x + cw, :3])) for j, (i, x, y, _, _) in
                    enumerate(crops))
    tc, tf = [], []
    for _ in range(runs):
        tc.append(wall_ms(torch, lambda: nice.decode_set(iset, windows=crops, out=batch, ctx=ctx)))
        tf.append(wall_ms(torch, lambda: nice.decode_set(iset, out=outs, ctx=ctx)))
    report["crop_batch"] = {"windows": K, "window": f"{cw}x{cw}", "tile": f"{tile[0]}x{tile[1]}",
                            "tiles_decoded": nc.value + nr.value, "tiles_in_set": iset.first[-1],
                            "crops": summary(tc), "full_decode_set": summary(tf),
                            "crop_phases": phases(lambda: nice.decode_set(iset, windows=crops, out=batch, ctx=ctx))}
    del iset, batch

    # ---- 3. the default tile
    sweep = []
    for tw, th in SWEEP:
        iset = nice.encode_set(imgs, tile=(tw, th), ctx=ctx)
        nice.decode_set(iset, out=outs, ctx=ctx)
        te, td = [], []
        for _ in range(runs):
            te.append(wall_ms(torch, lambda: nice.encode_set(imgs, tile=(tw, th), ctx=ctx)))
            td.append(wall_ms(torch, lambda: nice.decode_set(iset, out=outs, ctx=ctx)))
        ok = ok and exact()
        n = iset.first[-1]
        sweep.append({"tile": f"{tw}x{th}", "tiles": n, "raw_tiles": int(iset.kind.sum()), "packed_bytes": iset.nbytes,
                      "container_bytes": 48 + 8 * K + 8 * n + 8 * (n + 1) + n + (-n % 8) + iset.nbytes,
                      "encode_set": summary(te), "decode_set": summary(td),
                      "decode_set_phases": phases(lambda: nice.decode_set(iset, out=outs, ctx=ctx))})
        del iset
    report["tile_sweep"] = sweep
    del imgs, outs
    torch.cuda.empty_cache()

    # ---- 2. the copies of one large image
    if not args.skip_copies:
        W = H = 8192
        tw, th = 1024, 512
        px = bench.syn_frames(torch, 1, W, H, 1, dev)
        out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
        whole = torch.empty(W * H * 4, dtype=torch.uint8, device=dev)
        nx, ny = nice.tile_grid(W, H, tw, th)
        n, tstride = nx * ny, tw * th * 4
        tiles = torch.empty(n * tstride, dtype=torch.uint8, device=dev)
        tiles2 = torch.empty(n * tstride, dtype=torch.uint8, device=dev)
        idx = torch.arange(n, dtype=torch.int32, device=dev)
        zero = torch.zeros(n, dtype=torch.int32, device=dev)
        p = ctypes.c_void_p
        u32, u64 = ctypes.c_uint32, ctypes.c_uint64
        h_w, h_h = (u32 * 1)(W), (u32 * 1)(H)
        h_img, h_pitch = (p * 1)(px.data_ptr()), (u64 * 1)(W * 4)
        h_win, h_out, h_opitch = (u32 * 5)(0, 0, 0, W, H), (p * 1)(out.data_ptr()), (u64 * 1)(W * 4)

        def st():
            return p(torch.cuda.current_stream().cuda_stream)

        def split():
            assert L.nice_tiles_split_dev(ctx.ptr, st(), p(px.data_ptr()), W * 4, W, H, 4, tw, th, p(tiles.data_ptr()),
                                          tstride) == 0

        def set_split():
            assert L.nice_set_split_dev(ctx.ptr, st(), h_img, h_pitch, h_w, h_h, 1, 4, tw, th, p(tiles2.data_ptr()),
                                        tstride) == 0

        def merge():
            assert L.nice_tiles_merge_dev(ctx.ptr, st(), p(tiles.data_ptr()), tstride, p(idx.data_ptr()), n, 4, W, H, tw,
                                          th, 0, 0, W, H, 4, 0, p(out.data_ptr()), W * 4) == 0

        def set_merge():
            assert L.nice_set_merge_dev(ctx.ptr, st(), p(tiles.data_ptr()), tstride, None, p(zero.data_ptr()),
                                        p(idx.data_ptr()), None, n, 4, h_w, h_h, 1, tw, th, h_win, h_out, h_opitch, 1, 4,
                                        0) == 0

        def copy():
            whole.copy_(px.view(-1))

        fns = {"copy": copy, "tiles_split": split, "set_split": set_split, "tiles_merge": merge, "set_merge": set_merge}
        split()
        set_split()
        ok = ok and bool(torch.equal(tiles, tiles2))
        out.zero_()
        set_merge()
        ok = ok and bool(torch.equal(out.view(-1), px.view(-1)))
        for fn in fns.values():
            fn()
        tt = {k: [] for k in fns}
        for _ in range(runs):
            for k, fn in fns.items():
                tt[k].append(event_ms(torch, fn))
        cs = {k: summary(v) for k, v in tt.items()}

        def no_slower(a, b):
            return a["median_ms"] <= b["median_ms"] + max(a["spread_ms"], b["spread_ms"])

        report["copies_8192x8192_at_1024x512"] = dict(
            cs, bytes_moved=2 * W * H * 4,
            set_split_no_slower=no_slower(cs["set_split"], cs["tiles_split"]),
            set_merge_no_slower=no_slower(cs["set_merge"], cs["tiles_merge"]))

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
