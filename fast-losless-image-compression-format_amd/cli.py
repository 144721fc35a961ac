"""Command-line front end, mirroring the reference binary (main.rs:17-139):

    python fast-losless-image-compression-format_amd/cli.py IN.png OUT[.nice]
    python fast-losless-image-compression-format_amd/cli.py IN.nice OUT[.png]

A .png input (8-bit RGB or RGBA, main.rs:42-46) is encoded with channels_out =
its channel count (main.rs:66) and written to OUT, ".nice" appended when
missing (main.rs:59-61).  A .nice input is decoded and written as an RGB PNG
(main.rs:106-127), ".png" appended when missing.  The codec runs on the GPU
through libnice_hip.so.  Streams the reference decoder cannot read (4-channel
headers, spilled table headers of small/flat images) are decoded with the
tolerant options; --strict refuses them as the reference would.  Timings are
printed like the reference's (milliseconds).

Tiled images (this project's own container, lossless for every input):

    python fast-losless-image-compression-format_amd/cli.py IN.png OUT --tile WxH [--alpha]
    python fast-losless-image-compression-format_amd/cli.py IN.nicet OUT[.png] [--roi X,Y,W,H]

--tile writes OUT.nicet (".nicet" appended when missing); a .nicet input is
decoded, whole or the --roi rectangle alone, and written as an RGB PNG.
--alpha (an RGBA .png) also stores the alpha channel; a .nicet that holds one
is written as an RGBA PNG.

Image sets (many images of different sizes in one container):

    python fast-losless-image-compression-format_amd/cli.py --set DIR OUT[.nices] [--tile WxH] [--alpha]
    python fast-losless-image-compression-format_amd/cli.py IN.nices DIR
    python fast-losless-image-compression-format_amd/cli.py IN.nices OUT.png --index I

--set encodes the 8-bit RGB or RGBA PNGs of DIR (all of one kind, in the order
of their sorted names) as one set; a .nices input is decoded into DIR as
000000.png, 000001.png, ..., or image I alone into OUT.png.  --alpha (RGBA
PNGs) also stores the alpha channels; a .nices that holds them is written as
RGBA PNGs.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import time

import numpy as np


def _pkg():
    # the package directory name has hyphens: load it by path
    here = os.path.dirname(os.path.abspath(__file__))
    name = "fast-losless-image-compression-format_amd"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(here, "__init__.py"),
                                                  submodule_search_locations=[here])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--strict", action="store_true", help="decode only what the reference decoder can")
    ap.add_argument("--tile", metavar="WxH", help="encode a .png as a tiled image (.nicet) with tiles of W x H pixels")
    ap.add_argument("--roi", metavar="X,Y,W,H", help="decode only this rectangle of a .nicet")
    ap.add_argument("--alpha", action="store_true", help="with --tile or --set: keep the alpha channel of RGBA .png input")
    ap.add_argument("--set", action="store_true", help="encode the .png files of directory SRC as one image set (.nices)")
    ap.add_argument("--index", type=int, metavar="I", help="decode image I of a .nices into a .png")
    args = ap.parse_args(argv)
    try:
        tile = tuple(int(v) for v in args.tile.lower().split("x")) if args.tile else None
        roi = tuple(int(v) for v in args.roi.split(",")) if args.roi else None
        if (tile and len(tile) != 2) or (roi and len(roi) != 4):
            raise ValueError
    except ValueError:
        ap.error("--tile takes WxH, --roi takes X,Y,W,H")
    if roi and not args.src.endswith(".nicet"):
        ap.error("--roi needs a .nicet input")
    if tile and not args.src.endswith(".png") and not args.set:
        ap.error("--tile needs a .png input")
    if args.alpha and not tile and not args.set:
        ap.error("--alpha needs --tile or --set")
    if args.index is not None and not args.src.endswith(".nices"):
        ap.error("--index needs a .nices input")
    nice = _pkg()
    png = importlib.import_module(nice.__name__ + ".png")
    dst = args.dst
    print(f"a_file_from: {args.src}")
    print(f"a_file_to: {dst}")
    if args.set:
        import torch
        names = sorted(f for f in os.listdir(args.src) if f.endswith(".png"))
        imgs = [png.read_png(os.path.join(args.src, f)) for f in names]
        if not imgs or len({ch for _, _, _, ch in imgs}) != 1:
            print("--set needs a directory of .png files, all RGB or all RGBA", file=sys.stderr)
            return 2
        if args.alpha and imgs[0][3] != 4:
            print("--alpha needs RGBA .png files", file=sys.stderr)
            return 2
        if not dst.endswith(".nices"):
            dst += ".nices"
        t1 = time.perf_counter()
        iset = nice.encode_set([torch.from_numpy(np.array(px, np.uint8).reshape(h, w, ch)).cuda()
                                for px, w, h, ch in imgs], tile=tile, alpha=args.alpha)
        print(f"{(time.perf_counter() - t1) * 1e3:.0f}")
        nice.save_set(dst, iset)
        print(f"images: {len(iset)} tiles: {iset.first[-1]} raw: {int(iset.kind.sum())} bytes: {iset.nbytes}")
        if iset.alpha is not None:
            k = iset.alpha.kind
            print(f"alpha tiles: coded: {int((k == 0).sum())} raw: {int((k == 1).sum())} "
                  f"constant: {int((k == 2).sum())} bytes: {iset.alpha.nbytes}")
        return 0
    if args.src.endswith(".nices"):
        iset = nice.load_set(args.src, device="cuda")
        t0 = time.perf_counter()
        oc = 3 if iset.alpha is None else 4
        outs = nice.decode_set(iset, images=None if args.index is None else [args.index], out_channels=oc)
        rgbs = [o.cpu().numpy() for o in outs]
        print(f"nice elapsed in: {(time.perf_counter() - t0) * 1e3:.0f}")
        if args.index is not None:
            paths = [dst if dst.endswith(".png") else dst + ".png"]
        else:
            os.makedirs(dst, exist_ok=True)
            paths = [os.path.join(dst, f"{i:06d}.png") for i in range(len(rgbs))]
        for path, rgb in zip(paths, rgbs):
            png.write_png(path, rgb.reshape(-1, oc), rgb.shape[1], rgb.shape[0], oc)
        return 0
    if args.src.endswith(".png") and tile:
        import torch
        t0 = time.perf_counter()
        px, w, h, ch = png.read_png(args.src)
        print(f"png: {(time.perf_counter() - t0) * 1e3:.0f}")
        if args.alpha and ch != 4:
            print("--alpha needs an RGBA .png", file=sys.stderr)
            return 2
        if not dst.endswith(".nicet"):
            dst += ".nicet"
        print(f"bytes length: {px.size}")
        t1 = time.perf_counter()
        timg = nice.encode_tiled(torch.from_numpy(np.array(px, np.uint8).reshape(h, w, ch)).cuda(), tile=tile,
                                 alpha=args.alpha)
        print(f"{(time.perf_counter() - t1) * 1e3:.0f}")
        nice.save_tiled(dst, timg)
        print(f"tiles: {timg.nx}x{timg.ny} raw: {int(timg.kind.sum())} bytes: {timg.nbytes}")
        if timg.alpha is not None:
            k = timg.alpha.kind
            print(f"alpha tiles: coded: {int((k == 0).sum())} raw: {int((k == 1).sum())} "
                  f"constant: {int((k == 2).sum())} bytes: {timg.alpha.nbytes}")
        return 0
    if args.src.endswith(".nicet"):
        timg = nice.load_tiled(args.src, device="cuda")
        oc = 3 if timg.alpha is None else 4
        t0 = time.perf_counter()
        out = nice.decode_tiled(timg, roi=roi, out_channels=oc)
        rgb = out.cpu().numpy()
        print(f"nice elapsed in: {(time.perf_counter() - t0) * 1e3:.0f}")
        if not dst.endswith(".png"):
            dst += ".png"
        t1 = time.perf_counter()
        png.write_png(dst, rgb.reshape(-1, oc), rgb.shape[1], rgb.shape[0], oc)
        print(f"png{(time.perf_counter() - t1) * 1e3:.0f}")
        return 0
    if args.src.endswith(".png"):
        t0 = time.perf_counter()
        px, w, h, ch = png.read_png(args.src)
        print(f"png: {(time.perf_counter() - t0) * 1e3:.0f}")
        if not dst.endswith(".nice"):
            dst += ".nice"
        print(f"bytes length: {px.size}")
        out = bytearray()
        t1 = time.perf_counter()
        nice.encode(px, nice.Image.new(w, h, ch), ch, out)
        print(f"{(time.perf_counter() - t1) * 1e3:.0f}")
        with open(dst, "wb") as fh:
            fh.write(out)
        print(f"read png file: {args.src}")
        return 0
    if args.src.endswith(".nice"):
        data = open(args.src, "rb").read()
        t0 = time.perf_counter()
        flags = nice.DEC_STRICT_REFERENCE if args.strict else (nice.DEC_TOLERANT_HEADER | nice.DEC_ALPHA_FILL_FF)
        px, img = nice.decode_bytes(data, flags)
        print(f"nice elapsed in: {(time.perf_counter() - t0) * 1e3:.0f}")
        if not dst.endswith(".png"):
            dst += ".png"
        rgb = np.frombuffer(px, np.uint8).reshape(-1, img.channels)[:, :3]
        t1 = time.perf_counter()
        png.write_png(dst, rgb, img.width, img.height, 3)
        print(f"png{(time.perf_counter() - t1) * 1e3:.0f}")
        return 0
    print("input must be a .png, a .nice, a .nicet or a .nices file", file=sys.stderr)
    return 2


if __name__ == "__main__":
    sys.exit(main())
