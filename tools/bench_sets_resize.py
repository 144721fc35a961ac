#!/usr/bin/env python3
"""Timing of decode_set_resized (include/nice.h, "image sets: resized tensor
output") on one GPU, by the method of tools/bench_sets_tensor.py.

The workload: K RGBA SYN-v1 images of 256 x 256 generated on the device and
encoded as one set at the default tile; M = K windows, one per image, drawn
with a fixed seed in the random-resized-crop ranges (area 0.08 .. 1 of the
image, aspect 3/4 .. 4/3, log-uniform), all resampled to 224 x 224, every
second one mirrored, with the ImageNet constants.

The other side is the only other means to the same end: decode_set into M uint8
tensors of M different shapes, then, per window, the torch chain (permute,
float, interpolate(bilinear, antialias=False), normalise, flip, cast) written
into the batch.  Both sides are alternated in one run.

1. the merge stage alone, on the same pre-decoded 4-byte slots (HIP events):
   nice_set_resize_tensor_dev against nice_set_merge_dev plus the chain; the
   resize kernel's bytes read and written per second beside a device copy of the
   same byte count, from single calls and from 20 calls back to back;
2. end to end (all calls block: wall clock between device syncs):
   decode_set_resized against decode_set plus the chain;
3. torch's peak allocation on both sides.

float16, planar and channels_last, with the two bars.  Every figure is a median
of --runs with min, max and spread (max - min).

    python tools/bench_sets_resize.py [--images 256] [--runs 7] [--log profiles/sets_resize_bench.json]

--antialias adds the antialiased leg ("image sets: antialiased resized tensor
output") to the same run, sides alternated as above: decode_set_resized(
antialias=True) and nice_set_resize_aa_tensor_dev against the same chain with
interpolate(antialias=True), whose largest difference from the kernel is
checked per window against the bound derived from the definition; and, with no
bar, against the sampled call and kernel, beside the device copy, with the
peak allocations.  The bar: the antialiased call is faster than its chain end
to end by more than the sum of the two spreads.

    python tools/bench_sets_resize.py --antialias --log profiles/sets_resize_aa_bench.json
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = "fast-losless-image-compression-format_amd"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SIDE, CW = 256, 224


def random_resized_crop(rng, w, h):
    """torchvision's RandomResizedCrop.get_params with its default ranges."""
    for _ in range(10):
        area = w * h * rng.uniform(0.08, 1.0)
        aspect = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        rw, rh = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
        if 0 < rw <= w and 0 < rh <= h:
            return int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh
    return 0, 0, w, h


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--log", default=None, help="also write the report to this file")
    ap.add_argument("--antialias", action="store_true", help="add the antialiased leg")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import bench
    from bench_sets import event_ms, wall_ms, summary, wins
    nice = importlib.import_module(PKG)
    L = nice.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = nice.Context(0)
    K, runs = args.images, args.runs
    tw, th = nice.DEFAULT_SET_TILE
    rng = np.random.default_rng(21)
    imgs = [bench.syn_frames(torch, 1, SIDE, SIDE, 1 + i, dev).view(SIDE, SIDE, 4) for i in range(K)]
    crops = [(i,) + random_resized_crop(rng, SIDE, SIDE) for i in range(K)]
    M = len(crops)
    flips = [j % 2 for j in range(M)]
    scale, bias = nice.normalize_affine(MEAN, STD)
    iset = nice.encode_set(imgs, tile=(tw, th), ctx=ctx)
    areas = [rw * rh for _, _, _, rw, rh in crops]
    report = {"device": torch.cuda.get_device_name(dev), "images": K, "image": f"{SIDE}x{SIDE}", "tile": f"{tw}x{th}",
              "windows": M, "size": f"{CW}x{CW}", "flipped": sum(flips), "scale": list(scale), "bias": list(bias),
              "window_area_min_median_max": [min(areas), int(np.median(areas)), max(areas)],
              "crops": "numpy default_rng(21): area 0.08..1 of the image, aspect 3/4..4/3 log-uniform, then the position"}
    ok = True
    s_t = torch.tensor(scale, dtype=torch.float32, device=dev)
    b_t = torch.tensor(bias, dtype=torch.float32, device=dev)

    # ---- the torch chain behind M uint8 windows [rh, rw, 3], into out [M, 3, CW, CW]
    def chain(u8s, out, antialias=False):
        for j, u8 in enumerate(u8s):
            x = u8.permute(2, 0, 1)[None].float()
            x = F.interpolate(x, size=(CW, CW), mode="bilinear", align_corners=False, antialias=antialias)
            x = x.mul(s_t[None, :, None, None]).add(b_t[None, :, None, None])
            if flips[j]:
                x = x.flip(-1)
            out[j] = x[0].to(out.dtype)
        return out

    # ---- pre-decoded slots of the windows in position order: 4 bytes per pixel, dense
    stride = tw * th * 4
    slot_win, slot_tile, tiles = [], [], []
    nx = -(-SIDE // tw)
    for j, (i, x0, y0, rw, rh) in enumerate(crops):
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
    d_src = torch.arange(ns, dtype=torch.int64, device=dev)          # dense, slot p at p * stride
    p, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    h_w, h_h = (u32 * K)(*([SIDE] * K)), (u32 * K)(*([SIDE] * K))
    h_win = (u32 * (5 * M))(*[v for c in crops for v in c])
    h_flip = (ctypes.c_uint8 * M)(*flips)
    c_scale, c_bias = (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias)

    def st():
        return p(torch.cuda.current_stream().cuda_stream)

    def resize_fn(out, channels_last, entry="nice_set_resize_tensor_dev"):
        """out [M, 3, CW, CW], planar or a channels_last view"""
        es = out.element_size()
        base, step = out.data_ptr(), out.stride(0) * es
        h_out = (p * M)(*[base + j * step for j in range(M)])
        h_rp, h_pp = (u64 * M)(*([3 * CW if channels_last else CW] * M)), (u64 * M)(*([CW * CW] * M))
        layout = nice.TENSOR_INTERLEAVED if channels_last else nice.TENSOR_PLANAR

        def call():
            rc = getattr(L, entry)(
                ctx.ptr, st(), p(slots.data_ptr()), stride, None, p(d_src.data_ptr()), None, h_w, h_h, K, tw, th, h_win,
                h_flip, CW, CW, h_out, h_rp, h_pp, M, nice.TENSOR_F16, layout, c_scale, c_bias)
            assert rc == 0, rc
        return call

    u8s = [torch.empty((rh, rw, 3), dtype=torch.uint8, device=dev) for _, _, _, rw, rh in crops]
    h_u8 = (p * M)(*[t.data_ptr() for t in u8s])
    h_u8p = (u64 * M)(*[3 * c[3] for c in crops])

    def merge_u8():
        rc = L.nice_set_merge_dev(ctx.ptr, st(), p(slots.data_ptr()), stride, None, p(d_win.data_ptr()),
                                  p(d_tile.data_ptr()), None, ns, 4, h_w, h_h, K, tw, th, h_win, h_u8, h_u8p, M, 3, 0)
        assert rc == 0, rc

    def each_of(n, fn):
        def call():
            for _ in range(n):
                fn()
        return call

    def alloc(channels_last):
        if channels_last:
            return torch.empty((M, CW, CW, 3), dtype=torch.float16, device=dev).permute(0, 3, 1, 2)
        return torch.empty((M, 3, CW, CW), dtype=torch.float16, device=dev)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        keep = fn()
        torch.cuda.synchronize()
        got = torch.cuda.max_memory_allocated(dev) - base
        del keep
        return got

    def same_bits(a, b):
        return bool(torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)))

    def axis_bound(n_in):
        """grey levels one axis adds against the exact filter (tests/test_sets_resize_aa_cpu.py): a reducing
        axis of at most T taps 255 (T - 1) / 8192, T <= 2 ceil(n_in / CW) (the pixel centres inside an open interval 2 n_in / CW long); any other 255 / 512"""
        return 255 / 512 if CW >= n_in else 255 * (2 * -(-n_in // CW) - 1) / 8192

    def aa_leg(out, other, cl, resize, ca, cb, moved):
        kw = dict(windows=crops, size=(CW, CW), scale=scale, bias=bias, flip=flips, ctx=ctx)
        resize_aa = resize_fn(out, cl, "nice_set_resize_aa_tensor_dev")
        out.zero_()
        resize_aa()
        alone = out.clone()
        out.zero_()
        nice.decode_set_resized(iset, out=out, antialias=True, **kw)
        e2e_ok = same_bits(out, alone)
        merge_u8()
        chain(u8s, other, True)
        diff = (out.float() - other.float()).abs().amax(dim=(2, 3)).cpu().numpy()            # [M, 3]
        smax = np.abs(np.array(scale))
        bound = np.array([[(axis_bound(rw) + axis_bound(rh) + 2.0 ** -16) * s + 2 * 2.0 ** -11 * 3.0 for s in smax]
                          for _, _, _, rw, rh in crops])                                       # |v| < 3 with these constants
        chain_ok = bool((diff < bound).all())
        t = {k: [] for k in ("merge_aa", "merge_sampled", "merge_aa_chain", "copy", "e2e_aa", "e2e_sampled",
                             "e2e_aa_chain")}
        for _ in range(runs):
            t["merge_aa"].append(event_ms(torch, resize_aa))
            t["merge_sampled"].append(event_ms(torch, resize))
            t["merge_aa_chain"].append(event_ms(torch, lambda: (merge_u8(), chain(u8s, other, True))))
            t["copy"].append(event_ms(torch, lambda: cb.copy_(ca)))
            t["e2e_aa"].append(wall_ms(torch, lambda: nice.decode_set_resized(iset, out=out, antialias=True, **kw)))
            t["e2e_sampled"].append(wall_ms(torch, lambda: nice.decode_set_resized(iset, out=out, **kw)))
            t["e2e_aa_chain"].append(wall_ms(torch, lambda: chain(nice.decode_set(iset, windows=crops, out=u8s, ctx=ctx),
                                                                  other, True)))
        s = {k: summary(v) for k, v in t.items()}
        bar = (s["e2e_aa_chain"]["median_ms"] - s["e2e_aa"]["median_ms"]
               > s["e2e_aa_chain"]["spread_ms"] + s["e2e_aa"]["spread_ms"])
        return dict(
            s, windows_reducing_on_an_axis=sum(1 for c in crops if c[3] > CW or c[4] > CW),
            merge_aa_gb_s=round(moved / s["merge_aa"]["median_ms"] / 1e6, 1),
            copy_gb_s=round(moved / s["copy"]["median_ms"] / 1e6, 1),
            merge_aa_over_sampled=round(s["merge_aa"]["median_ms"] / s["merge_sampled"]["median_ms"], 2),
            e2e_aa_over_sampled=round(s["e2e_aa"]["median_ms"] / s["e2e_sampled"]["median_ms"], 3),
            e2e_ratio=round(s["e2e_aa_chain"]["median_ms"] / s["e2e_aa"]["median_ms"], 3),
            peak_bytes_aa=peak(lambda: nice.decode_set_resized(iset, channels_last=cl, antialias=True, **kw)),
            peak_bytes_chain=peak(lambda: chain(nice.decode_set(iset, windows=crops, out_channels=3, ctx=ctx), alloc(cl),
                                                True)),
            decode_bits_equal_kernels_alone=e2e_ok, chain_within_bound=chain_ok,
            largest_difference_to_chain=diff.max(axis=0).tolist(), largest_bound=bound.max(axis=0).tolist(),
            bar_e2e_aa_faster_than_chain_by_more_than_both_spreads=bool(bar),
            checks_passed=e2e_ok and chain_ok and bool(bar))               # the bar decides the exit status too

    REPS = 20
    for name, cl in (("float16", False), ("float16_channels_last", True)):
        out, other = alloc(cl), alloc(cl)
        resize = resize_fn(out, cl)
        # checks: the kernel alone and the whole call give the same bits; the chain is within the bound of the
        # definition (|scale| * 255/256 in output units) plus the float16 roundings of both sides
        out.zero_()
        resize()
        alone = out.clone()
        out.zero_()
        nice.decode_set_resized(iset, windows=crops, size=(CW, CW), out=out, scale=scale, bias=bias, flip=flips, ctx=ctx)
        e2e_ok = same_bits(out, alone)
        merge_u8()
        u8_ok = all(bool(torch.equal(u, imgs[i][y0:y0 + rh, x0:x0 + rw, :3])) for u, (i, x0, y0, rw, rh) in zip(u8s, crops))
        chain(u8s, other)
        diff = (out.float() - other.float()).abs().amax(dim=(0, 2, 3)).tolist()
        bound = [abs(s) * 255 / 256 + 2 * 2.0 ** -11 * 3.0 for s in scale]       # |v| < 3 with these constants
        chain_ok = all(d < b for d, b in zip(diff, bound))
        ok = ok and e2e_ok and u8_ok and chain_ok
        moved = 4 * sum(areas) + M * 3 * CW * CW * 2
        ca = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        cb = torch.empty_like(ca)
        t = {k: [] for k in ("merge_resize", "merge_chain", "copy", "merge_resize_back_to_back", "copy_back_to_back",
                             "e2e_resized", "e2e_chain")}
        for _ in range(runs):
            t["merge_resize"].append(event_ms(torch, resize))
            t["merge_chain"].append(event_ms(torch, lambda: (merge_u8(), chain(u8s, other))))
            t["copy"].append(event_ms(torch, lambda: cb.copy_(ca)))
            t["merge_resize_back_to_back"].append(event_ms(torch, each_of(REPS, resize)) / REPS)
            t["copy_back_to_back"].append(event_ms(torch, each_of(REPS, lambda: cb.copy_(ca))) / REPS)
            t["e2e_resized"].append(wall_ms(torch, lambda: nice.decode_set_resized(
                iset, windows=crops, size=(CW, CW), out=out, scale=scale, bias=bias, flip=flips, ctx=ctx)))
            t["e2e_chain"].append(wall_ms(torch, lambda: chain(nice.decode_set(iset, windows=crops, out=u8s, ctx=ctx),
                                                               other)))
        s = {k: summary(v) for k, v in t.items()}
        report[name] = dict(
            s, bytes_read_and_written_by_resize=moved,
            merge_resize_gb_s=round(moved / s["merge_resize"]["median_ms"] / 1e6, 1),
            copy_gb_s=round(moved / s["copy"]["median_ms"] / 1e6, 1),
            merge_resize_back_to_back_gb_s=round(moved / s["merge_resize_back_to_back"]["median_ms"] / 1e6, 1),
            copy_back_to_back_gb_s=round(moved / s["copy_back_to_back"]["median_ms"] / 1e6, 1),
            merge_ratio=round(s["merge_chain"]["median_ms"] / s["merge_resize"]["median_ms"], 2),
            e2e_ratio=round(s["e2e_chain"]["median_ms"] / s["e2e_resized"]["median_ms"], 3),
            peak_bytes_resized=peak(lambda: nice.decode_set_resized(
                iset, windows=crops, size=(CW, CW), scale=scale, bias=bias, flip=flips, channels_last=cl, ctx=ctx)),
            peak_bytes_chain=peak(lambda: chain(nice.decode_set(iset, windows=crops, out_channels=3, ctx=ctx), alloc(cl))),
            decode_bits_equal_kernel_alone=e2e_ok, uint8_merge_exact=u8_ok, chain_within_bound=chain_ok,
            largest_difference_to_chain=diff, bound=bound,
            # the rules of DESIGN.md: a win needs median + spread below the other's median - spread;
            # not slower means median <= the other's median + its spread
            bar_merge_resize_wins=wins(s["merge_resize"], s["merge_chain"]),
            bar_e2e_not_slower=s["e2e_resized"]["median_ms"] <= s["e2e_chain"]["median_ms"] + s["e2e_chain"]["spread_ms"])
        if args.antialias:
            report[name]["antialias"] = aa_leg(out, other, cl, resize, ca, cb, moved)
            ok = ok and report[name]["antialias"]["checks_passed"]
        del out, other, alone, ca, cb

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
