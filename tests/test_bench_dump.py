"""bench.py --dump-outputs / --full: the dump's layout and determinism on the
CPU (dump_outputs on host tensors, the stand-in step), and on the GPU a small
plain run whose dumped stream lengths and checksums must be the oracle's, and a
small --full run that must still fill the legs a plain run leaves out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args,
                         capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def _sums(b):
    v = np.frombuffer(bytes(b), np.uint8).astype(np.int64)
    return [int(v.sum()), int((v * (np.arange(v.size) % 65521 + 1)).sum())]


def test_dump_outputs_layout(tmp_path):
    import torch
    import bench
    rng = np.random.default_rng(3)
    F, stride, npx = 11, 70001, 66000
    streams = torch.from_numpy(rng.integers(0, 256, (F, stride), dtype=np.uint8))
    dec = torch.from_numpy(rng.integers(0, 256, (F, npx), dtype=np.uint8))
    lens = torch.from_numpy(rng.integers(1, stride + 1, F).astype(np.int64))
    lens[4] = 0
    lens[7] = stride
    status = torch.zeros(F, dtype=torch.int32)
    bench.dump_outputs(torch, str(tmp_path / "a"), streams, lens, dec, status)
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")}
    assert set(a) == {"lens", "status", "stream_sums", "decoded_sums", "stream_sample", "decoded_sample"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.array_equal(a["lens"], lens.numpy()) and not a["status"].any()
    for f in range(F):
        assert list(a["stream_sums"][f]) == _sums(streams[f, :int(lens[f])].numpy())
        assert list(a["decoded_sums"][f]) == _sums(dec[f].numpy())
    k = min(F, bench.DUMP_FRAMES)
    assert a["stream_sample"].shape == a["decoded_sample"].shape == (k, min(bench.DUMP_BYTES, npx))
    assert (a["stream_sample"] == -1).all(axis=1).sum() <= 1            # only frame 4's empty stream
    assert ((a["decoded_sample"] >= 0) & (a["decoded_sample"] <= 255)).all()
    # bytes past a stream's length are not output: changing them changes nothing;
    # changing any output byte does
    s2 = streams.clone()
    for f in range(F):
        s2[f, int(lens[f]):] ^= 0xFF
    bench.dump_outputs(torch, str(tmp_path / "b"), s2, lens, dec, status)
    for n, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / (n + ".npy"))), n
    d2 = dec.clone()
    d2[F - 1, npx - 1] ^= 1
    bench.dump_outputs(torch, str(tmp_path / "c"), streams, lens, d2, status)
    assert not np.array_equal(a["decoded_sums"], np.load(tmp_path / "c" / "decoded_sums.npy"))


def test_standin_dump_repeats(tmp_path):
    got = []
    for d in ("a", "b"):
        res = _bench(["--standin", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / d)])
        assert res["steps"] == 2 and res["ms_per_step"] > 0
        got.append(np.load(tmp_path / d / "standin.npy"))
    assert got[0].dtype == np.float64 and np.array_equal(got[0], got[1])


W, H, F = 320, 200, 3
SMALL = ["--gpus", "1", "--frames", str(F), "--width", str(W), "--height", str(H)]


@pytest.mark.gpu
def test_plain_run_dumps_the_oracles_streams(tmp_path, O):
    res = _bench(SMALL + ["--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert all(k in res for k in KEYS)
    assert res["steps"] == 2 and res["warmup"] == 1 and res["unit"] == "MPixels/s" and res["dtype"] == "u8"
    # value is the pixels of a step over ms_per_step (printed to 0.001 ms, value to 0.001)
    tol = 0.0005 / (res["ms_per_step"] - 0.0005) + 1e-9
    assert abs(res["value"] - F * W * H / (res["ms_per_step"] * 1e-3) / 1e6) <= tol * res["value"] + 0.001
    # a plain run leaves every side measurement out
    for k in ("stream_check", "cpu_baseline", "cpu_baseline_threads", "rgb_4k", "config3_batch_1080p",
              "uhd8k_7680x4320", "sharded_image_encode", "streamed_host_frames", "subblock_positions",
              "encode_mpix_s", "decode_mpix_s", "single_frame_latency_ms"):
        assert res[k] is None, k
    a = {n[:-4]: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    assert not a["status"].any()
    for f in range(F):
        px = O.gen_syn_v1(W, H, 4, 1 + f)
        want = O.encode(px, W, H, 4)
        assert a["lens"][f] == len(want)
        assert list(a["stream_sums"][f]) == _sums(want)
        rgb = int(px.reshape(-1, 4)[:, :3].astype(np.int64).sum())
        assert a["decoded_sums"][f][0] - rgb in (0, 255 * W * H)        # RGB exact; alpha filled 0 or 255
    assert a["stream_sample"].min() >= 0 and a["stream_sample"].max() <= 255


@pytest.mark.gpu
def test_full_run_fills_the_side_legs():
    res = _bench(SMALL + ["--steps", "1", "--warmup", "1", "--full", "--rgb-frames", "2", "--config3-frames", "0",
                          "--uhd8k-frames", "0", "--streamed-frames", "0", "--sharded-side", "0",
                          "--cpu-seconds", "0.2"])
    assert all(k in res for k in KEYS)
    assert "byte-exact" in res["stream_check"]
    assert res["cpu_baseline"]["value"] > 0 and res["cpu_baseline_threads"]["value"] > 0
    assert res["rgb_4k"]["stream_check"] and res["encode_mpix_s"] > 0 and res["decode_mpix_s"] > 0
    assert res["roofline"]["copy_peak_measured"] > 0 and res["subblock_positions"]["ms"] > 0
