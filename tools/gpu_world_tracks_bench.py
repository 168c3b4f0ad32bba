#!/usr/bin/env python3
"""Parity figures and timing of bt_world_tracks (world-frame point cloud, 3-D track trajectories, overwrite of the live
tracks' window buffer) -> profiles/r10_world_tracks.txt.

Parity: the figures tests/test_gpu_world_tracks.py asserts on — per fixture case the reference's own float32 error e32 and
the kernel's error per output, the fused kernel against the composed operations at the two test sizes, and the replayed
caller's feedback figures.

Timing: device events around every single call, warm-up first, the fused call and the path composed from the operations
the package had before (pops.point_cloud, pops.proj, SE3 gather / inverse / action; tests/world_util.py) alternating in
one process; median and 10 % / 90 % quantiles.  Sizes: Sintel 50 x 256, DAVIS 50 x 400 and the full buffer 1023 x 256
tracks, S_slam 12 (S_local 23), about 70 % live tracks.  Algorithmic bytes from the shapes: per slot 12 (patches_local
read) + 4 (weight) + 12 (world written), + 12 for a live track's slot (patches_local written); per track 12 (patch) + 8 (ix)
+ 12 (point); over the median time, as a share of the HBM peak.  The working set of the full buffer (0.25 GB) fits the
256 MiB Infinity Cache in part, so repeated calls need not come from HBM: the share is of the HBM peak all the same.

    python tools/gpu_world_tracks_bench.py [--reps 200] [--out profiles/r10_world_tracks.txt] [--no-parity]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_world_tracks_bench.py --trace     (a run of its own)
    python tools/gpu_world_tracks_bench.py --trace-db DIR/.../*_results.db --out FILE     (appends the kernel's times per size)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import world_util as wu  # noqa: E402
from batrack_amd import _lib  # noqa: E402
from batrack_amd.backend.lietorch import SE3  # noqa: E402

HBM_PEAK = 8.0e12                                            # B/s, spec
SIZES = (("Sintel 50 x 256", 51, 256, 50), ("DAVIS 50 x 400", 51, 400, 50), ("full buffer 1023 x 256", 1024, 256, 1023))
S_SLAM = 12
DEV = "cuda:0"


def algorithmic_bytes(m, S, live_tracks):
    return m * S * (12 + 4 + 12) + live_tracks * S * 12 + m * (12 + 8 + 12)


def per_call_us(fns, reps, warmup=20):
    """Each of `fns` called `reps` times, alternating, an event pair around every call: {name: array of us}."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in fns}
    for r in range(reps):
        for k, f in fns.items():
            a, b = ev[k][r]
            a.record()
            f()
            b.record()
    torch.cuda.synchronize()
    return {k: np.array([a.elapsed_time(b) * 1e3 for a, b in v]) for k, v in ev.items()}


def setup(N, M, n):
    d = wu.random_inputs(N, M, S_SLAM, n, seed=N + M)
    g = wu.to_gpu(d, DEV)
    live = int((d["local_weights"][:g["m"]].sum(1) > 0).sum())
    NM, S = g["patches_local"].shape[1:3]
    pl = g["patches_local"].clone()
    points = torch.zeros(NM, 3, device=DEV)
    world = torch.zeros(1, NM, S, 3, device=DEV)
    P = g["poses"][0].contiguous()
    # (the operator itself: the Python wrapper's reshapes would be timed as device idle time between the two events)
    ops, pat, K, plv, lw = _lib.torch_ops(strict=True), g["patches"][0], g["intrinsics"][0], pl[0], g["local_weights"]
    fused = lambda: ops.world_tracks(P, pat, K, g["ix"], plv, lw, g["m"], points, world)
    composed = lambda: wu.composed_world_tracks(SE3, g["poses"], g["patches"], g["intrinsics"], g["ix"], g["patches_local"],
                                                g["local_weights"], g["m"])
    return g, live, S, fused, composed


def parity(out):
    D = dict(np.load(wu.GOLD))
    np64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    out("parity against the reference's float64 run (tests/golden/world_tracks.npz); e32 = the reference's own float32 run, gate = 2 x e32;")
    out("(u, v) on the project's gate |got - ref| / (100 + |ref|) < 2e-5")
    for c in wu.CASES:
        d = wu.fixture_case(D, c)
        m = int(d["m"])
        p, w, o = wu.run_fused(wu.to_gpu(d, DEV))
        f = wu.parity_figures((np64(p), np64(w)[0], np64(o)[0]), (D[f"{c}.points"], D[f"{c}.world"], D[f"{c}.patches_local_out"]), m,
                              d["local_weights"][:m].sum(1) > 0, D[f"{c}.near_clamp"])
        out(f"  case {c}: " + "  ".join(f"{k} e32 {float(D[f'gate.{c}.{k}']):.3e} kernel {f[k]:.3e}" for k in ("points", "world", "disp"))
            + f"  uv kernel {f['uv']:.3e} (share compared {f['uv_share']:.3f})  finiteness equal {f['finite']}  untouched rows equal {f['rest']}")
    out("fused against the composed operations (both float32 on the GPU), gate 2 x e32 of case a:")
    for _, N, M, n in (SIZES[0], SIZES[2]):
        d = wu.random_inputs(N, M, S_SLAM, n, seed=N + M)
        g = wu.to_gpu(d, DEV)
        a = wu.run_fused(g)
        b = wu.composed_world_tracks(SE3, g["poses"], g["patches"], g["intrinsics"], g["ix"], g["patches_local"], g["local_weights"], g["m"])
        f = wu.parity_figures((np64(a[0]), np64(a[1])[0], np64(a[2])[0]), (np64(b[0]), np64(b[1])[0], np64(b[2])[0]), g["m"],
                              d["local_weights"][:g["m"]].sum(1) > 0)
        out(f"  N {N} M {M} m {g['m']}: " + "  ".join(f"{k} {f[k]:.3e}" for k in ("points", "world", "disp", "uv"))
            + f"  finiteness equal {f['finite']}  untouched rows equal {f['rest']}")
    f = wu.caller_feedback(DEV)
    out("replayed caller, 24 frames x 32 tracks, UPDATE_POINT_CLOUD: largest pose difference fused / composed run "
        f"{f['pose_diff']:.3e}; largest relative deviation of a live track's depth prior from its disparity after the last update: "
        f"fused {f['dev_fused']:.3e}, composed {f['dev_composed']:.3e}, default replay (step off) {f['dev_default']:.3e}; live tracks {f['live']} of {f['m']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_world_tracks.txt"))
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--trace", action="store_true", help="20 fused and 5 composed calls per size, nothing written: for rocprofv3")
    ap.add_argument("--trace-db", help="append this kernel's times per size from a rocprofv3 results database, then exit")
    args = ap.parse_args()
    if args.trace_db:
        import sqlite3
        rows = sqlite3.connect(args.trace_db).cursor().execute(
            "select grid_x, end - start from kernels where name like '%k_world_tracks%' order by start").fetchall()
        with open(args.out, "a") as fh:
            fh.write("kernel time, rocprofv3 --kernel-trace --stats in a run of its own (23 fused calls per size, the first 3 left out):\n")
            grids = list(dict.fromkeys(r[0] for r in rows))                      # one launch shape per size, in SIZES' order
            for (name, N, M, n), grid in zip(SIZES, grids):
                m, S = n * M, 2 * S_SLAM - 1
                t = np.array([r[1] for r in rows if r[0] == grid][3:]) / 1e3
                by = algorithmic_bytes(m, S, int(0.7 * m))
                fh.write(f"  {name}: grid {grid} threads, {len(t)} calls, k_world_tracks median {np.median(t):.2f} us (min {t.min():.2f}, max {t.max():.2f}); "
                         f"{by / 1e6:.1f} MB algorithmic at 70 % live = {by / np.median(t) / 1e3:.0f} GB/s = "
                         f"{100 * by / (np.median(t) * 1e-6) / HBM_PEAK:.1f} % of the HBM peak\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is measured without one")
    if args.trace:
        for _, N, M, n in SIZES:
            _, _, _, fused, composed = setup(N, M, n)
            for _ in range(23):
                fused()
            for _ in range(5):
                composed()
            torch.cuda.synchronize()
        return
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"bt_world_tracks on {torch.cuda.get_device_name(0)}; S_slam {S_SLAM}, S_local {2 * S_SLAM - 1}; HBM peak {HBM_PEAK / 1e12:.1f} TB/s (spec)")
    if not args.no_parity:
        parity(out)
    out(f"timing: device events around each call, {args.reps} calls each, fused and composed alternating; us median [10 % .. 90 %]")
    for name, N, M, n in SIZES:
        g, live, S, fused, composed = setup(N, M, n)
        t = per_call_us(dict(fused=fused, composed=composed), args.reps)
        q = {k: np.quantile(v, [0.5, 0.1, 0.9]) for k, v in t.items()}
        by = algorithmic_bytes(g["m"], S, live)
        out(f"  {name}: m {g['m']} tracks ({live / g['m']:.0%} live), {g['m'] * S} slots, {by / 1e6:.1f} MB algorithmic; "
            f"fused {q['fused'][0]:.1f} [{q['fused'][1]:.1f} .. {q['fused'][2]:.1f}] us = {by / q['fused'][0] / 1e3:.0f} GB/s = "
            f"{100 * by / (q['fused'][0] * 1e-6) / HBM_PEAK:.1f} % of the HBM peak; composed {q['composed'][0]:.1f} "
            f"[{q['composed'][1]:.1f} .. {q['composed'][2]:.1f}] us; composed / fused {q['composed'][0] / q['fused'][0]:.1f}x")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
