#!/usr/bin/env python3
"""Timing of the mono-depth alignment (main/mono_depth/get_mono_depth.py:52-140) on the device (bt_mono_align) against numpy
on the host, in one run:
  sizes 50 x 480 x 854 (DAVIS) and 50 x 436 x 1024 (Sintel), float32 and float64 metric depth (the disparity is float32);
  the device time is the median of per-call CUDA-event times over --reps warm calls; the algorithmic bytes are what the
  passes read and write (rounds A, B, C: d and m once per 8-bit digit; the percentile round: d once per digit; the write:
  d in, the depth out), against the 8 TB/s HBM peak (the inputs fit the 256 MiB Infinity Cache: the passes after the first
  read it there);
  the host time is the numpy restatement (tests/mono_util.py, bit-equal to the reference on its fixture) timed once; the
  device result is checked bit-equal to it (equal_nan) at each size, with the scales, shifts, aligns and k.
Run a second time under rocprofv3 --kernel-trace --stats (with --no-host) for the per-kernel times.

    python tools/gpu_mono_depth_bench.py [--reps 30] [--no-host] [--out profiles/r09_mono_depth.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from batrack_amd.mono_depth import align_mono_depth  # noqa: E402
from mono_util import restate  # noqa: E402

HBM_PEAK = 8.0e12


def scene(T, H, W, dt, seed=0):
    """DepthAnything-like disparity in (0, 1) with a sky band below 0.01, UniDepth-like depth ~ 1 / (a d + b) with noise."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, H, dtype=np.float32), np.linspace(0, 1, W, dtype=np.float32), indexing="ij")
    d = np.empty((T, H, W), np.float32)
    m = np.empty((T, H, W), dt)
    for t in range(T):
        base = 0.02 + 0.9 * (0.5 + 0.5 * np.sin(2.5 * x + 1.5 * y + 0.1 * t))
        dd = base * (1 + np.float32(0.05) * rng.standard_normal((H, W), np.float32))
        dd[: H // 8] = np.float32(0.005)
        d[t] = dd
        m[t] = 1 / (rng.uniform(0.5, 2) * dd + 0.05) * (1 + 0.03 * rng.standard_normal((H, W)))
    return d, m


def algorithmic_bytes(n, es):
    passes = es                                       # 8-bit digits of a D key
    return 3 * passes * (4 + es) * n + passes * 4 * n + (4 + es) * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    head = (f"device {torch.cuda.get_device_name(0)}; host threads: OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')}; "
            f"numpy {np.__version__}")
    print(head, flush=True)
    rows = []
    for name, (T, H, W) in (("DAVIS", (50, 480, 854)), ("Sintel", (50, 436, 1024))):
        for dt in (np.float32, np.float64):
            d, m = scene(T, H, W, dt)
            dg, mg = torch.as_tensor(d, device=dev), torch.as_tensor(m, device=dev)
            out = torch.empty_like(mg)
            for _ in range(3):
                align_mono_depth(dg, mg, out=out)
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
            for a, b in ev:
                a.record()
                align_mono_depth(dg, mg, out=out)
                b.record()
            torch.cuda.synchronize()
            times = sorted(a.elapsed_time(b) for a, b in ev)
            ms = float(np.median(times))
            n, es = d.size, np.dtype(dt).itemsize
            nb = algorithmic_bytes(n, es)
            row = {"scene": name, "T": T, "H": H, "W": W, "dtype": np.dtype(dt).name, "device_ms_median": round(ms, 4),
                   "device_ms_min": round(times[0], 4), "device_ms_max": round(times[-1], 4), "calls": args.reps,
                   "algorithmic_bytes": nb, "GB_per_s": round(nb / ms / 1e6, 1), "hbm_peak_share": round(nb / (ms * 1e-3) / HBM_PEAK, 3)}
            line = (f"{name:6s} {T} x {H} x {W} {np.dtype(dt).name}: device {ms:7.3f} ms median ({times[0]:.3f} .. {times[-1]:.3f}, "
                    f"{args.reps} calls); {nb / 1e9:.2f} GB algorithmic = {nb / ms / 1e6:7.1f} GB/s = "
                    f"{100 * nb / (ms * 1e-3) / HBM_PEAK:.0f} % of the HBM peak")
            if not args.no_host:
                t0 = time.perf_counter()
                ref, rs, rc, ral, rk = restate(d, m)
                th = time.perf_counter() - t0
                got, s, c, al, k = align_mono_depth(dg, mg, return_stats=True)
                eq = lambda a, b: bool(a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True))
                same = (eq(got.cpu().numpy(), ref) and eq(s.cpu().numpy(), rs) and eq(c.cpu().numpy(), rc)
                        and eq(al.cpu().numpy(), ral) and k == rk)
                row.update(host_numpy_ms=round(th * 1e3, 1), ratio=round(th * 1e3 / ms, 1), bit_equal=same, k=k)
                line += f"; host numpy {th * 1e3:8.1f} ms ({th * 1e3 / ms:.0f}x); bit-equal: {same}"
            rows.append(row)
            print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"header": head, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
