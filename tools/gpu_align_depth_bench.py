#!/usr/bin/env python3
"""Timing of align_depth_maps (main/global_refine/model/utils.py:268-312) on the device (bt_align_depth_maps) against the host
function, in one run:
  the host function `_align_depth_maps` (numpy, bit-equal to the reference's) on this machine's host;
  bt_align_depth_maps warm, by CUDA events over repeated calls (the whole chain of one scene per call);
  cases: 50 x 436 x 1024 float64 (results.pkl's dtype) and float32, and a DAVIS-like 90 x 480 x 854 float64;
  the wall time of RefineLosses.from_results(align_depth=True) on a synthetic Sintel-size results dictionary, with the
  maps aligned on the host (the dictionary's maps pre-aligned by `_align_depth_maps`, then align_depth=False: what
  from_results did before) against the device path, each outcome checked bit-equal.
Run a second time under rocprofv3 --kernel-trace --stats (with --no-host) for the per-kernel times.

    python tools/gpu_align_depth_bench.py [--reps 20] [--no-host]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from batrack_amd.global_refine import RefineLosses, _align_depth_maps, align_depth_maps_device  # noqa: E402


def scene(T, H, W, dtype, seed=0):
    """Mono-depth-like maps: smooth positive depth with a per-frame scale drift, 3 % invalid (0) pixels."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = 2.0 + 8.0 * (0.5 + 0.5 * np.sin(3 * x + 2 * y))
    maps = np.empty((T, H, W, 1), dtype)
    for t in range(T):
        d = base * rng.uniform(0.5, 2.0) * (1 + 0.1 * rng.standard_normal((H, W)))
        d[rng.random((H, W)) < 0.03] = 0.0
        maps[t, ..., 0] = d
    return maps


def results_dict(maps, N=256, S=11, seed=1):
    T, H, W = maps.shape[:3]
    rng = np.random.default_rng(seed)
    t2d = np.concatenate([rng.uniform(0, W - 1, (T, N, S, 1)), rng.uniform(0, H - 1, (T, N, S, 1)), rng.uniform(0.1, 1.0, (T, N, S, 1))], -1)
    cams = np.tile(np.eye(4), (T, 1, 1))
    cams[:, :3, 3] = rng.normal(0.0, 0.1, (T, 3))
    return {"trajs_2d_disp": t2d.astype(np.float32), "cams_T_world": cams.astype(np.float32),
            "intrinsics": np.tile(np.array([500.0, 500.0, W / 2, H / 2], np.float32), (T, 1)),
            "trajs_vis": np.ones((T, N, S), np.float32), "trajs_static": np.ones((T, N, S), np.float32),
            "trajs_valid": np.ones((T, N), bool), "grid_query_frames": np.arange(0, T, 2), "dmaps": maps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    dev = "cuda:0"
    print(f"device {torch.cuda.get_device_name(0)}; host threads: OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')}; numpy {np.__version__}")
    for T, H, W, dt in ((50, 436, 1024, np.float64), (50, 436, 1024, np.float32), (90, 480, 854, np.float64)):
        maps = scene(T, H, W, dt)
        x = torch.as_tensor(maps[..., 0], device=dev)
        out = torch.empty_like(x)
        call = lambda: align_depth_maps_device(x, out=out)
        call()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            call()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / args.reps
        line = f"{T} x {H} x {W} {np.dtype(dt).name}: device {ms:7.2f} ms per scene (events, warm, {args.reps} calls)"
        if not args.no_host:
            t0 = time.perf_counter()
            ref = _align_depth_maps(maps)
            th = time.perf_counter() - t0
            same = np.array_equal(out.cpu().numpy(), ref[..., 0])
            line += f"; host _align_depth_maps {th * 1e3:8.1f} ms ({th * 1e3 / ms:.0f}x); bit-equal: {same}"
        print(line, flush=True)

    maps = scene(50, 436, 1024, np.float64)
    res = results_dict(maps)
    kw = dict(grid_size=12, loss_weight_dict={"spatial_loss": 5.0, "inter_frame_loss": 0.3, "pts_3d_loss": 1.0})
    RefineLosses.from_results(dict(res), dev, align_depth=True, **kw)               # warm: code objects, allocator
    torch.cuda.synchronize()
    walls = {}
    for tag in ("host", "device"):
        t0 = time.perf_counter()
        if tag == "host":
            net = RefineLosses.from_results(dict(res, dmaps=_align_depth_maps(maps)), dev, align_depth=False, **kw)
        else:
            net = RefineLosses.from_results(dict(res), dev, align_depth=True, **kw)
        torch.cuda.synchronize()
        walls[tag] = (time.perf_counter() - t0, net)
    same = torch.equal(walls["host"][1].dmaps, walls["device"][1].dmaps) and \
        torch.equal(walls["host"][1].trajs_disp_mono, walls["device"][1].trajs_disp_mono)
    print(f"from_results(align_depth=True), 50 x 436 x 1024 float64, wall: host alignment {walls['host'][0] * 1e3:8.1f} ms, "
          f"device alignment {walls['device'][0] * 1e3:8.1f} ms; dmaps and trajs_disp_mono bit-equal: {same}")


if __name__ == "__main__":
    main()
