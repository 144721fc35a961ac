#!/usr/bin/env python3
"""Timing of the packed stream batch (include/nice.h, "packed stream batches")
on one GPU, with HIP events:

* pack throughput: nice_pack_streams_dev on a batch of SYN-v1 streams,
  (bytes read + bytes written) / time, beside a torch copy_ of the same byte
  count measured in the same run;
* decode through the offset table against the strided decode of the same
  streams, alternated, median and spread of each;
* footprint: off[n] against n x out_stride.

    python tools/packed_timing.py [--frames 512] [--width 3840] [--height 2160] [--runs 12] [--log FILE]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "fast-losless-image-compression-format_amd"


def timed_ms(torch, fn, runs, warmup=2):
    """Per-run times of fn() between two events on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def summary(ts):
    s = sorted(ts)
    return {"median_ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4),
            "runs": len(s)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--log", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import torch
    import bench
    nice = importlib.import_module(PKG)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, W, H = args.frames, args.width, args.height

    px = bench.syn_frames(torch, n, W, H, 1, dev)
    stride = (nice.encode_bound(W, H) + 255) // 256 * 256
    streams = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    lens = torch.zeros(n, dtype=torch.int64, device=dev)
    nice.encode_batch(px, W, H, 4, streams, lens)
    torch.cuda.synchronize()
    hl = lens.cpu().tolist()
    total = sum((l + 15) // 16 * 16 for l in hl)
    packed = torch.empty(total, dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    pstatus = torch.zeros(1, dtype=torch.int32, device=dev)

    # ---- pack against a plain copy of the same byte count
    t_pack = timed_ms(torch, lambda: nice.pack_streams(streams, lens, packed, off, pstatus), args.runs)
    assert int(pstatus[0]) == 0 and int(off[n]) == total
    flat_src = streams.view(-1)[:total]
    flat_dst = torch.empty(total, dtype=torch.uint8, device=dev)
    t_copy = timed_ms(torch, lambda: flat_dst.copy_(flat_src), args.runs)
    read_bytes = sum((l + 3) // 4 * 4 for l in hl)
    pack_gbs = (read_bytes + total) / (statistics.median(t_pack) * 1e-3) / 1e9
    copy_gbs = 2 * total / (statistics.median(t_copy) * 1e-3) / 1e9

    # ---- decode: strided and packed alternated
    del px   # (the two decodes are compared with each other below)
    dec_s = torch.empty((n, W * H * 4), dtype=torch.uint8, device=dev)
    dec_p = torch.zeros((n, W * H * 4), dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    status_p = torch.ones(n, dtype=torch.int32, device=dev)

    def strided():
        nice.decode_batch(streams, lens, W, H, 4, dec_s, status, host_len=hl)

    def from_packed():
        nice.decode_batch_packed(packed, off, lens, W, H, 4, dec_p, status_p, host_len=hl, packed_bytes=total)

    for fn in (strided, from_packed):   # warm both (scratch sized, code loaded)
        fn()
    torch.cuda.synchronize()
    t_s, t_p = [], []
    for _ in range(args.runs):
        t_s += timed_ms(torch, strided, 1, warmup=0)
        t_p += timed_ms(torch, from_packed, 1, warmup=0)
    torch.cuda.synchronize()
    # the two routes decode the same pixels
    same = bool((status == 0).all()) and bool((status_p == 0).all()) and torch.equal(dec_s, dec_p)

    report = {
        "device": torch.cuda.get_device_name(dev),
        "batch": f"{n} x {W}x{H} RGBA SYN-v1 streams",
        "footprint": {"packed_bytes": total, "strided_bytes": n * stride,
                      "ratio": round(total / (n * stride), 4)},
        "pack": dict(summary(t_pack), bytes_read=read_bytes, bytes_written=total, gb_s=round(pack_gbs, 1)),
        "copy_same_bytes": dict(summary(t_copy), gb_s=round(copy_gbs, 1)),
        "pack_vs_copy": round(pack_gbs / copy_gbs, 3),
        "decode_strided": summary(t_s),
        "decode_packed": summary(t_p),
        "decode_median_diff_ms": round(statistics.median(t_p) - statistics.median(t_s), 4),
        "decode_outputs_equal": same,
    }
    text = json.dumps(report, indent=1)
    print(text)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)) or ".", exist_ok=True)
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0 if report["decode_outputs_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
