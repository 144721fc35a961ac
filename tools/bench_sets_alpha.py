#!/usr/bin/env python3
"""Timing of the alpha batch of image sets (include/nice.h, "image sets: alpha")
on one GPU, by the method of tools/bench_sets.py.  The workload is that tool's:
K RGBA SYN-v1 images generated on the device, widths and heights from the same
fixed-seed list between 256 and 1536.  Byte +3 is filled in two ways: all
opaque (255), and a soft-edged disc per image (255 inside, 0 outside, a ramp of
24 pixels between), so that only the tiles the edge crosses are coded.

1. the bar, per filling: encode_set(alpha=True) and decode_set of that set
   against the only other means to the same end, a loop of
   encode_tiled(alpha=True) / decode_tiled over the same images at the same
   tile size, alternated in one run (all four calls block: wall clock between
   device syncs);
2. the opaque set: alpha=True against alpha=False, encode and decode, alternated;
3. the kernels: a one-image set of 8192 x 8192 RGBA at 1024 x 512, the set range
   pass beside nice_tiles_alpha_range_dev, and the set alpha merge beside the
   tiled one (every tile a raw plane, so neither call decodes), on the 16-byte
   path (HIP events, alternated).

Every figure is a median of --runs with min, max and spread (max - min).

    python tools/bench_sets_alpha.py [--images 256] [--runs 7] [--tile 256x256] [--log profiles/sets_alpha_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = "fast-losless-image-compression-format_amd"

from bench_sets import N_PHASES, FIRST_DEC_PHASE, event_ms, summary, wall_ms, wins   # noqa: E402


def disc_alpha(torch, w, h, dev):
    """255 inside a centred disc of radius 0.3 * min(w, h), 0 outside, 24 pixels of ramp."""
    y = torch.arange(h, device=dev, dtype=torch.float32)[:, None] - h / 2
    x = torch.arange(w, device=dev, dtype=torch.float32)[None, :] - w / 2
    d = torch.sqrt(x * x + y * y)
    return torch.clamp((0.3 * min(w, h) + 12 - d) * (255 / 24), 0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--tile", default=None, help="tile of parts 1 and 2 (default: DEFAULT_SET_TILE)")
    ap.add_argument("--skip-kernels", action="store_true", help="leave out part 3 (8192 x 8192)")
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
              "tile": f"{tile[0]}x{tile[1]}",
              "sizes": "RGBA SYN-v1 seeds 1.., widths and heights numpy default_rng(20).integers(256, 1537)"}
    ok = True

    def exact():
        return all(bool(torch.equal(o, im)) for o, im in zip(outs, imgs))

    def dec_phases(fn):
        L.nice_ctx_set_timing(ctx.ptr, 1)
        t = wall_ms(torch, fn)
        ms, cnt = (ctypes.c_double * N_PHASES)(), (ctypes.c_uint32 * N_PHASES)()
        L.nice_ctx_read_timing(ctx.ptr, ms, cnt)
        L.nice_ctx_set_timing(ctx.ptr, 0)
        d = {L.nice_phase_name(i).decode(): round(ms[i], 3) for i in range(FIRST_DEC_PHASE, N_PHASES)}
        d["launches_of_dec_tables"] = cnt[FIRST_DEC_PHASE]
        d["wall_ms"] = round(t, 3)
        return d

    # ---- 1. the set against the loop, per filling; 2. the opaque set with and without alpha
    for filling in ("opaque", "disc"):
        for im, (w, h) in zip(imgs, sizes):
            im[:, :, 3] = 255 if filling == "opaque" else disc_alpha(torch, w, h, dev)
        iset = nice.encode_set(imgs, tile=tile, ctx=ctx, alpha=True)                # warm: scratch sized
        timgs = [nice.encode_tiled(im, tile=tile, ctx=ctx, alpha=True) for im in imgs]
        t = {k: [] for k in ("encode_set", "encode_loop", "decode_set", "decode_loop")}
        for _ in range(runs):
            t["encode_set"].append(wall_ms(torch, lambda: nice.encode_set(imgs, tile=tile, ctx=ctx, alpha=True)))
            t["encode_loop"].append(wall_ms(torch, lambda: [nice.encode_tiled(im, tile=tile, ctx=ctx, alpha=True)
                                                            for im in imgs]))
            for o in outs:
                o.zero_()
            t["decode_set"].append(wall_ms(torch, lambda: nice.decode_set(iset, out=outs, flags=0, ctx=ctx)))
            ok = ok and exact()
            for o in outs:
                o.zero_()
            t["decode_loop"].append(wall_ms(torch, lambda: [nice.decode_tiled(ti, out=o, flags=0, ctx=ctx)
                                                            for ti, o in zip(timgs, outs)]))
            ok = ok and exact()
        s = {k: summary(v) for k, v in t.items()}
        a = iset.alpha
        same = all(bool(torch.equal(ti.alpha.packed, a.packed[int(a.off[lo]):int(a.off[hi])]))
                   and ti.alpha.kind.tolist() == a.kind[lo:hi].tolist()
                   for ti, lo, hi in zip(timgs, iset.first[:-1], iset.first[1:]))
        ok = ok and same
        report[f"bar_{filling}"] = dict(
            s, tiles=iset.first[-1], alpha_coded=int((a.kind == 0).sum()), alpha_raw=int((a.kind == 1).sum()),
            alpha_constant=int((a.kind == 2).sum()), alpha_bytes=a.nbytes, colour_bytes=iset.nbytes,
            set_equals_concatenated_tiled_alpha=same,
            decode_set_wins=wins(s["decode_set"], s["decode_loop"]),
            encode_set_wins=wins(s["encode_set"], s["encode_loop"]),
            decode_speedup=round(s["decode_loop"]["median_ms"] / s["decode_set"]["median_ms"], 2),
            encode_speedup=round(s["encode_loop"]["median_ms"] / s["encode_set"]["median_ms"], 2),
            decode_set_phases=dec_phases(lambda: nice.decode_set(iset, out=outs, flags=0, ctx=ctx)))
        del timgs
        if filling == "opaque":
            plain = nice.encode_set(imgs, tile=tile, ctx=ctx)
            t = {k: [] for k in ("encode_alpha", "encode_plain", "decode_alpha", "decode_plain")}
            for _ in range(runs):
                t["encode_alpha"].append(wall_ms(torch, lambda: nice.encode_set(imgs, tile=tile, ctx=ctx, alpha=True)))
                t["encode_plain"].append(wall_ms(torch, lambda: nice.encode_set(imgs, tile=tile, ctx=ctx)))
                t["decode_alpha"].append(wall_ms(torch, lambda: nice.decode_set(iset, out=outs, flags=0, ctx=ctx)))
                t["decode_plain"].append(wall_ms(torch, lambda: nice.decode_set(plain, out=outs, ctx=ctx)))
            s = {k: summary(v) for k, v in t.items()}
            report["opaque_alpha_against_plain"] = dict(
                s, encode_ratio=round(s["encode_alpha"]["median_ms"] / s["encode_plain"]["median_ms"], 3),
                decode_ratio=round(s["decode_alpha"]["median_ms"] / s["decode_plain"]["median_ms"], 3))
            del plain
        del iset
    del imgs, outs
    torch.cuda.empty_cache()

    # ---- 3. the kernels on one large image
    if not args.skip_kernels:
        W = H = 8192
        tw, th = 1024, 512
        px = bench.syn_frames(torch, 1, W, H, 1, dev).view(H, W, 4)
        px[:, :, 3] = disc_alpha(torch, W, H, dev)
        nx, ny = nice.tile_grid(W, H, tw, th)
        n, npx = nx * ny, tw * th
        p = ctypes.c_void_p
        u32, u64 = ctypes.c_uint32, ctypes.c_uint64
        h_w, h_h = (u32 * 1)(W), (u32 * 1)(H)
        h_img, h_pitch = (p * 1)(px.data_ptr()), (u64 * 1)(W * 4)
        lo, hi = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        lo2, hi2 = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        # every tile a raw plane of random bytes: the merges read them, nothing is decoded
        planes = torch.randint(0, 256, (n * npx,), dtype=torch.uint8, device=dev)
        aoff = torch.arange(n + 1, dtype=torch.int64) * npx
        alen = torch.full((n,), npx, dtype=torch.int64)
        akind = torch.ones(n, dtype=torch.uint8)
        aval = torch.zeros(n, dtype=torch.uint8)
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
        out2 = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        h_win, h_out, h_opitch = (u32 * 5)(0, 0, 0, W, H), (p * 1)(out2.data_ptr()), (u64 * 1)(W * 4)
        tabs = [p(t.data_ptr()) for t in (aoff, alen, akind, aval)]

        def st():
            return p(torch.cuda.current_stream().cuda_stream)

        def alpha_range():
            assert L.nice_tiles_alpha_range_dev(ctx.ptr, st(), p(px.data_ptr()), W * 4, W, H, tw, th, p(lo.data_ptr()),
                                                p(hi.data_ptr())) == 0

        def set_alpha_range():
            assert L.nice_set_alpha_range_dev(ctx.ptr, st(), h_img, h_pitch, h_w, h_h, 1, tw, th, p(lo2.data_ptr()),
                                              p(hi2.data_ptr())) == 0

        def alpha_merge():
            assert L.nice_decode_tiled_alpha_dev(ctx.ptr, st(), p(planes.data_ptr()), n * npx, *tabs, W, H, tw, th, 0, 0,
                                                 W, H, p(out.data_ptr()), W * 4, p(status.data_ptr())) == 0

        def set_alpha_merge():
            assert L.nice_decode_set_alpha_dev(ctx.ptr, st(), p(planes.data_ptr()), n * npx, *tabs, h_w, h_h, 1, tw, th,
                                               h_win, h_out, h_opitch, 1, p(status.data_ptr())) == 0

        fns = {"alpha_range": alpha_range, "set_alpha_range": set_alpha_range, "alpha_merge": alpha_merge,
               "set_alpha_merge": set_alpha_merge}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        ok = ok and bool(torch.equal(lo, lo2)) and bool(torch.equal(hi, hi2)) and bool(torch.equal(out, out2))
        ok = ok and bool(torch.equal(out[:, :, 3].reshape(ny, th, nx, tw).permute(0, 2, 1, 3).reshape(-1), planes))
        tt = {k: [] for k in fns}
        for _ in range(runs):
            for k, fn in fns.items():
                tt[k].append(event_ms(torch, fn))
        cs = {k: summary(v) for k, v in tt.items()}

        def no_slower(a, b):
            return a["median_ms"] <= b["median_ms"] + a["spread_ms"] + b["spread_ms"]

        report["kernels_8192x8192_at_1024x512"] = dict(
            cs, range_bytes_read=W * H * 4, merge_bytes_moved=2 * W * H * 4 + W * H,
            set_alpha_range_no_slower=no_slower(cs["set_alpha_range"], cs["alpha_range"]),
            set_alpha_merge_no_slower=no_slower(cs["set_alpha_merge"], cs["alpha_merge"]))

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
