#!/usr/bin/env python3
"""Timing of decode_set_tensor (include/nice.h, "image sets: tensor output") on
one GPU.  The workload is tools/bench_sets.py's: K RGBA SYN-v1 images generated
on the device, widths and heights from the same fixed-seed list, encoded as one
set at the default tile; M = K windows of 224 x 224, one per image at a
fixed-seed position, every second one mirrored; the ImageNet constants.

The other side is the only other means to the same end: decode_set into a
[M, 224, 224, 3] uint8 batch, then the torch chain (permute, float, mul, add,
half) and the flip, done by torch.where or by an indexed flip, whichever is
faster in this run.  Both sides are alternated in one run.

1. the merge stage alone, on the same pre-decoded 4-byte slots (HIP events):
   nice_set_merge_tensor_dev against nice_set_merge_dev plus the chain, each a
   call with its table upload; the tensor merge's bytes per second beside a
   device copy of the same byte count, from single calls and from 20 calls
   back to back (the device's time per call, where the host enqueues faster);
2. end to end (all calls block: wall clock between device syncs):
   decode_set_tensor against decode_set plus the chain;
3. torch's peak allocation on both sides.

For float16, planar and channels_last, with the two bars; float32 and bfloat16
(planar) are reported without one.  Every figure is a median of --runs with
min, max and spread (max - min).

    python tools/bench_sets_tensor.py [--images 256] [--runs 7] [--log profiles/sets_tensor_bench.json]
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
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CW = 224


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--log", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch
    import bench
    from bench_sets import event_ms, wall_ms, summary, wins
    nice = importlib.import_module(PKG)
    L = nice.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = nice.Context(0)
    K, runs = args.images, args.runs
    tw, th = nice.DEFAULT_SET_TILE
    rng = np.random.default_rng(20)
    sizes = rng.integers(256, 1537, (K, 2)).tolist()
    imgs = [bench.syn_frames(torch, 1, w, h, 1 + i, dev).view(h, w, 4) for i, (w, h) in enumerate(sizes)]
    crops = [(i, int(rng.integers(0, w - CW + 1)), int(rng.integers(0, h - CW + 1)), CW, CW)
             for i, (w, h) in enumerate(sizes)]
    M = len(crops)
    flips = [j % 2 for j in range(M)]
    scale, bias = nice.normalize_affine(MEAN, STD)
    iset = nice.encode_set(imgs, tile=(tw, th), ctx=ctx)
    report = {"device": torch.cuda.get_device_name(dev), "images": K, "tile": f"{tw}x{th}", "windows": M,
              "window": f"{CW}x{CW}", "flipped": sum(flips), "scale": list(scale), "bias": list(bias),
              "sizes": "RGBA SYN-v1 seeds 1.., widths and heights numpy default_rng(20).integers(256, 1537)"}
    ok = True

    # the crops as uint8, from the images themselves: the truth of every check below
    truth = torch.stack([imgs[i][y:y + CW, x:x + CW, :3] for i, x, y, _, _ in crops])
    flip_mask = torch.tensor(flips, dtype=torch.bool, device=dev)
    flip_idx = torch.nonzero(flip_mask).view(-1)

    def expected(dtype):
        """The table lookup (tests/test_sets_tensor.py), [M, 3, CW, CW] planar."""
        b = np.arange(256, dtype=np.float64)[:, None]
        lut = (b * np.array(scale, np.float64)[None, :] + np.array(bias, np.float64)[None, :]).astype(np.float32)
        lut = torch.from_numpy(lut).to(dtype).to(dev)
        want = torch.stack([lut[:, c][truth[:, :, :, c].long()] for c in range(3)], dim=1)
        return torch.where(flip_mask[:, None, None, None], want.flip(-1), want)

    def same_bits(a, b):
        it = torch.int32 if a.element_size() == 4 else torch.int16
        return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))

    # ---- the torch chain behind a uint8 batch [M, CW, CW, 3]
    def chain(u8, dtype, channels_last, how):
        s = torch.tensor(scale, dtype=torch.float32, device=dev)
        t = torch.tensor(bias, dtype=torch.float32, device=dev)
        if channels_last:       # the cheaper order for this layout: no permute of the data
            x = u8.float().mul(s).add(t).to(dtype).permute(0, 3, 1, 2)
        else:
            x = u8.permute(0, 3, 1, 2).float().mul(s[None, :, None, None]).add(t[None, :, None, None]).to(dtype)
        if how == "where":
            return torch.where(flip_mask[:, None, None, None], x.flip(-1), x)
        x[flip_idx] = x[flip_idx].flip(-1)
        return x

    # ---- pre-decoded slots of the windows: 4 bytes per pixel, dense, as the batch decoder leaves them
    stride = tw * th * 4
    slot_win, slot_tile, tiles = [], [], []
    for j, (i, x0, y0, rw, rh) in enumerate(crops):
        w, h = sizes[i]
        nx = -(-w // tw)
        for ty in range(y0 // th, (y0 + rh - 1) // th + 1):
            for tx in range(x0 // tw, (x0 + rw - 1) // tw + 1):
                t = torch.zeros((th, tw, 4), dtype=torch.uint8, device=dev)
                part = imgs[i][ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
                t[:part.shape[0], :part.shape[1]] = part
                tiles.append(t.view(-1))
                slot_win.append(j)
                slot_tile.append(ty * nx + tx)
    ns = len(tiles)
    slots = torch.stack(tiles)
    del tiles
    d_win = torch.tensor(slot_win, dtype=torch.int32, device=dev)
    d_tile = torch.tensor(slot_tile, dtype=torch.int32, device=dev)
    p, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    h_w, h_h = (u32 * K)(*[w for w, _ in sizes]), (u32 * K)(*[h for _, h in sizes])
    h_win = (u32 * (5 * M))(*[v for c in crops for v in c])
    h_flip = (ctypes.c_uint8 * M)(*flips)
    c_scale, c_bias = (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias)
    DT = {torch.float32: nice.TENSOR_F32, torch.float16: nice.TENSOR_F16, torch.bfloat16: nice.TENSOR_BF16}

    def st():
        return p(torch.cuda.current_stream().cuda_stream)

    # (the host tables of both merges are built once, outside the timed calls)
    def merge_tensor_fn(out, channels_last):
        """out [M, 3, CW, CW], planar or a channels_last view"""
        es = out.element_size()
        base, step = out.data_ptr(), out.stride(0) * es
        h_out = (p * M)(*[base + j * step for j in range(M)])
        h_rp, h_pp = (u64 * M)(*([3 * CW if channels_last else CW] * M)), (u64 * M)(*([CW * CW] * M))
        dt, layout = DT[out.dtype], nice.TENSOR_INTERLEAVED if channels_last else nice.TENSOR_PLANAR

        def call():
            rc = L.nice_set_merge_tensor_dev(
                ctx.ptr, st(), p(slots.data_ptr()), stride, None, p(d_win.data_ptr()), p(d_tile.data_ptr()), None, ns,
                4, h_w, h_h, K, tw, th, h_win, h_flip, h_out, h_rp, h_pp, M, dt, layout, c_scale, c_bias)
            assert rc == 0, rc
        return call

    def merge_u8_fn(u8):
        base, step = u8.data_ptr(), u8.stride(0)
        h_out, h_rp = (p * M)(*[base + j * step for j in range(M)]), (u64 * M)(*([3 * CW] * M))

        def call():
            rc = L.nice_set_merge_dev(
                ctx.ptr, st(), p(slots.data_ptr()), stride, None, p(d_win.data_ptr()), p(d_tile.data_ptr()), None, ns,
                4, h_w, h_h, K, tw, th, h_win, h_out, h_rp, M, 3, 0)
            assert rc == 0, rc
        return call

    def each_of(n, fn):
        """fn n times back to back: per call, the device's time where the host enqueues faster than it runs"""
        def call():
            for _ in range(n):
                fn()
        return call

    def alloc(dtype, channels_last):
        if channels_last:
            return torch.empty((M, CW, CW, 3), dtype=dtype, device=dev).permute(0, 3, 1, 2)
        return torch.empty((M, 3, CW, CW), dtype=dtype, device=dev)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        keep = fn()
        torch.cuda.synchronize()
        got = torch.cuda.max_memory_allocated(dev) - base
        del keep
        return got

    u8 = torch.empty((M, CW, CW, 3), dtype=torch.uint8, device=dev)
    merge_u8 = merge_u8_fn(u8)
    px = M * CW * CW
    REPS = 20
    configs = [("float16", torch.float16, False, True), ("float16_channels_last", torch.float16, True, True),
               ("float32", torch.float32, False, False), ("bfloat16", torch.bfloat16, False, False)]
    for name, dtype, cl, barred in configs:
        want = expected(dtype)
        out = alloc(dtype, cl)
        es = out.element_size()
        # checks: the merge alone and the whole call give the table's bits; the chain is close to them
        merge_tensor = merge_tensor_fn(out, cl)
        out.zero_()
        merge_tensor()
        merge_ok = same_bits(out, want)
        out.zero_()
        nice.decode_set_tensor(iset, windows=crops, out=out, dtype=dtype, scale=scale, bias=bias, flip=flips, ctx=ctx)
        e2e_ok = same_bits(out, want)
        u8.zero_()
        merge_u8()
        u8_ok = bool(torch.equal(u8, truth))
        tol = {torch.float32: 1e-5, torch.float16: 4e-3, torch.bfloat16: 3e-2}[dtype]
        chain_ok = all(bool((chain(u8, dtype, cl, how).float() - want.float()).abs().max() <= tol)
                       for how in ("where", "index"))
        ok = ok and merge_ok and e2e_ok and u8_ok and chain_ok
        # a device copy of the tensor merge's byte count (read 4 bytes per pixel, written 3 elements)
        moved = px * (4 + 3 * es)
        ca = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        cb = torch.empty_like(ca)
        t = {k: [] for k in ("merge_tensor", "merge_chain_where", "merge_chain_index", "copy", "merge_tensor_back_to_back",
                             "copy_back_to_back", "e2e_tensor", "e2e_chain_where", "e2e_chain_index")}
        for _ in range(runs):
            t["merge_tensor"].append(event_ms(torch, merge_tensor))
            t["merge_chain_where"].append(event_ms(torch, lambda: (merge_u8(), chain(u8, dtype, cl, "where"))))
            t["merge_chain_index"].append(event_ms(torch, lambda: (merge_u8(), chain(u8, dtype, cl, "index"))))
            t["copy"].append(event_ms(torch, lambda: cb.copy_(ca)))
            t["merge_tensor_back_to_back"].append(event_ms(torch, each_of(REPS, merge_tensor)) / REPS)
            t["copy_back_to_back"].append(event_ms(torch, each_of(REPS, lambda: cb.copy_(ca))) / REPS)
            t["e2e_tensor"].append(wall_ms(torch, lambda: nice.decode_set_tensor(
                iset, windows=crops, out=out, dtype=dtype, scale=scale, bias=bias, flip=flips, ctx=ctx)))
            for how in ("where", "index"):
                t["e2e_chain_" + how].append(wall_ms(torch, lambda: (
                    nice.decode_set(iset, windows=crops, out=u8, ctx=ctx), chain(u8, dtype, cl, how))))
        s = {k: summary(v) for k, v in t.items()}
        mc = min(("merge_chain_where", "merge_chain_index"), key=lambda k: s[k]["median_ms"])
        ec = min(("e2e_chain_where", "e2e_chain_index"), key=lambda k: s[k]["median_ms"])
        r = dict(s, bytes_moved_by_tensor_merge=moved,
                 merge_tensor_gb_s=round(moved / s["merge_tensor"]["median_ms"] / 1e6, 1),
                 copy_gb_s=round(moved / s["copy"]["median_ms"] / 1e6, 1),
                 merge_tensor_back_to_back_gb_s=round(moved / s["merge_tensor_back_to_back"]["median_ms"] / 1e6, 1),
                 copy_back_to_back_gb_s=round(moved / s["copy_back_to_back"]["median_ms"] / 1e6, 1),
                 merge_other_side=mc, e2e_other_side=ec,
                 merge_ratio=round(s[mc]["median_ms"] / s["merge_tensor"]["median_ms"], 2),
                 e2e_ratio=round(s[ec]["median_ms"] / s["e2e_tensor"]["median_ms"], 3),
                 peak_bytes_tensor=peak(lambda: nice.decode_set_tensor(
                     iset, windows=crops, dtype=dtype, scale=scale, bias=bias, flip=flips, channels_last=cl, ctx=ctx)),
                 peak_bytes_chain=peak(lambda: chain(nice.decode_set(
                     iset, windows=crops, out=torch.empty((M, CW, CW, 3), dtype=torch.uint8, device=dev), ctx=ctx),
                     dtype, cl, ec.rsplit("_", 1)[1])),
                 merge_bits_equal_table=merge_ok, decode_bits_equal_table=e2e_ok, uint8_merge_exact=u8_ok,
                 chain_within_tolerance=chain_ok)
        if barred:
            # the rules of DESIGN.md: a win needs median + spread below the other's median - spread;
            # not slower means median <= the other's median + its spread
            r["bar_merge_tensor_wins"] = wins(s["merge_tensor"], s[mc])
            r["bar_e2e_not_slower"] = s["e2e_tensor"]["median_ms"] <= s[ec]["median_ms"] + s[ec]["spread_ms"]
        report[name] = r
        del want, out, ca, cb

    report["all_checks_passed"] = ok
    text = json.dumps(report, indent=1)
    print(text)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)) or ".", exist_ok=True)
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
