#!/usr/bin/env python3
"""Timing of bt_observe_window (the step between the tracker's forward pass and the BA: targets, weights, pose weights,
patches_valid, query disparity, window buffers) -> profiles/r14_observe.txt.

One call at the Sintel shape (S 12, 6 keyframes x 256 = 1,536 queries, 436 x 1024 maps) and at the DAVIS shape (6 x 400 =
2,400 queries, 480 x 854), STATIC_QUANTILE 0.3 so that the quantile is interpolated.  Device events around every single
call, warm-up first; median and 10 % / 90 % quantiles.  Three forms on the same GPU, alternating in one process:
  fused      torch.ops.batrack_hip.observe_window (the operator itself), three launches;
  composed   the torch restatement tests/observe_util.window_observations_ref: the same arithmetic in tensor operations,
             the threshold fetched with `.item()` as the reference fetches it, the queries sampled in ONE vectorised call;
  per-query  the same with the queries sampled as the reference samples them: a Python loop over the queries, each
             iteration the bilinear sample of one query in tensor operations of one element (fewer repetitions: a call
             takes a large fraction of a second).
Before the timing the three forms are compared: every output and buffer bit for bit.

    python tools/gpu_observe_bench.py [--reps 200] [--loop-reps 5] [--out profiles/r14_observe.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_observe_bench.py --trace        (a run of its own)
    python tools/gpu_observe_bench.py --trace-db DIR/.../*_results.db --out FILE    (appends a line per kernel and shape)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import observe_util as ou  # noqa: E402
from batrack_amd import _lib  # noqa: E402
from batrack_amd.frontend.observe import ObserveConfig, window_observations  # noqa: E402

SHAPES = (("Sintel", 256, 436, 1024), ("DAVIS", 400, 480, 854))
S, KF = 12, 2
DEV = "cuda:0"
KERNELS = ("k_observe_query", "k_observe_threshold", "k_observe_window")


def sample_per_query(dmaps, queries):
    """sample_maps one query at a time, every step a tensor operation on one element, the results concatenated."""
    _, H, W = dmaps.shape
    out = []
    for i in range(queries.shape[0]):
        q = queries[i:i + 1]
        im = dmaps[q[:, 0].long()].reshape(-1)
        x, y = q[:, 1], q[:, 2]
        x0, y0 = torch.floor(x).int(), torch.floor(y).int()
        x1, y1 = x0 + 1, y0 + 1
        cx0, cx1 = torch.clamp(x0, 0, W - 1), torch.clamp(x1, 0, W - 1)
        cy0, cy1 = torch.clamp(y0, 0, H - 1) * W, torch.clamp(y1, 0, H - 1) * W
        i00, i01, i10, i11 = im[(cy0 + cx0).long()], im[(cy0 + cx1).long()], im[(cy1 + cx0).long()], im[(cy1 + cx1).long()]
        x0f, x1f, y0f, y1f = x0.float(), x1.float(), y0.float(), y1.float()
        w00, w01, w10, w11 = (x1f - x) * (y1f - y), (x - x0f) * (y1f - y), (x1f - x) * (y - y0f), (x - x0f) * (y - y0f)
        out.append(w00 * i00 + w01 * i01 + w10 * i10 + w11 * i11)
    return torch.cat(out)


def setup(M, H, W):
    Q = S // KF
    args, kw = ou.random_inputs(M, Q * M, M, S, S, KF, DEV, H=H, W=W, N=64, n=40, cfg=ObserveConfig(STATIC_QUANTILE=0.3))
    traj, depth, vis, dyn, queries, dmaps, ii, jj, kk = args
    ops = _lib.torch_ops(strict=True)
    ws = torch.empty(16, device=DEV)
    c = kw["cfg"]
    flat = (traj[0].contiguous(), depth.reshape(S, -1), vis[0], dyn[0], queries[0], dmaps, ii, jj, kk)
    bufs = [kw[k] for k in ("patches_valid",) + ou.BUFFERS]
    # (the operator itself: the Python wrapper's reshapes would be timed as device idle time between the two events)
    fused = lambda: ops.observe_window(*flat, *bufs, ws, kw["n"], S, KF, H, W, float(W), float(H), 20, c.VIS_THRESHOLD, c.STATIC_QUANTILE,
                                       c.STATIC_THRESHOLD, c.MIN_TRACK_LEN, True, 512, 384)
    composed = lambda: ou.window_observations_ref(*args, **kw)
    looped = lambda: ou.window_observations_ref(*args, **kw, sampler=sample_per_query)
    return args, kw, fused, composed, looped


def per_call_us(fns, reps, warmup):
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


def equal_forms(args, kw):
    res = []
    for f, extra in ((window_observations, {}), (ou.window_observations_ref, {}), (ou.window_observations_ref, dict(sampler=sample_per_query))):
        a, k = ou.clone_call(args, kw)
        res.append(ou.results(f(*a, **k, **extra), k))
    return all(ou.same_bits(res[0][k], r[k]) for r in res[1:] for k in ou.OUTPUTS)


def occupancy(vgpr, lds, wg):
    """Waves per SIMD the registers and the LDS allow (512 VGPRs a lane in steps of 8, 160 KiB LDS a CU, 4 SIMDs, at most 8)."""
    by_reg = min(8, 512 // max(8, -(-vgpr // 8) * 8))
    waves = max(1, wg // 64)
    by_lds = (160 * 1024 // lds) * waves / 4 if lds else 8
    return min(by_reg, by_lds, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--loop-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_observe.txt"))
    ap.add_argument("--trace", action="store_true", help="23 fused calls per shape, nothing written: for rocprofv3")
    ap.add_argument("--trace-db", help="append the kernels' times per shape from a rocprofv3 results database, then exit")
    args = ap.parse_args()
    if args.trace_db:
        import sqlite3
        cur = sqlite3.connect(args.trace_db).cursor()
        with open(args.out, "a") as fh:
            fh.write("kernel time, rocprofv3 --kernel-trace --stats in a run of its own (23 fused calls per shape, the first 3 left out); "
                     "waves per SIMD: what the registers and the LDS allow\n")
            for kn in KERNELS:
                rows = cur.execute("select grid_x, end - start, vgpr_count, sgpr_count, lds_size, workgroup_x from kernels "
                                   "where name like ? order by start", (f"%{kn}%",)).fetchall()
                grids = list(dict.fromkeys(r[0] for r in rows)) if kn != "k_observe_threshold" else [None]
                for (name, M, H, W), grid in zip(SHAPES if grids != [None] else (("both shapes",) + SHAPES[0][1:],), grids):
                    sel = [r for r in rows if grid is None or r[0] == grid]
                    t = np.array([r[1] for r in sel][3:]) / 1e3
                    _, _, vg, sg, lds, wg = sel[0]
                    fh.write(f"  {kn} {name}: grid {sel[0][0]} x workgroup {wg}, {len(t)} calls, median {np.median(t):.2f} us (min {t.min():.2f}, "
                             f"max {t.max():.2f}); {vg} VGPRs, {sg} SGPRs, {lds} B LDS, {occupancy(vg, lds, wg):g} waves per SIMD\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is measured without one")
    if args.trace:
        for _, M, H, W in SHAPES:
            fused = setup(M, H, W)[2]
            for _ in range(23):
                fused()
            torch.cuda.synchronize()
        return
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"bt_observe_window on {torch.cuda.get_device_name(0)}; S {S}, kf_stride {KF}, STATIC_QUANTILE 0.3, interp 512 x 384")
    out(f"timing: device events around each call, fused and composed alternating {args.reps} calls each, per-query {args.loop_reps} calls; "
        "us median [10 % .. 90 %]")
    for name, M, H, W in SHAPES:
        a, kw, fused, composed, looped = setup(M, H, W)
        same = equal_forms(a, kw)
        t = per_call_us(dict(fused=fused, composed=composed), args.reps, 20)
        t.update(per_call_us(dict(looped=looped), args.loop_reps, 1))
        q = {k: np.quantile(v, [0.5, 0.1, 0.9]) for k, v in t.items()}
        Nq = S // KF * M
        out(f"  {name}: Nq {Nq}, E {Nq * S}, maps {H} x {W}; the three forms bit-equal: {same}; "
            f"fused {q['fused'][0]:.1f} [{q['fused'][1]:.1f} .. {q['fused'][2]:.1f}] us; "
            f"composed {q['composed'][0]:.0f} [{q['composed'][1]:.0f} .. {q['composed'][2]:.0f}] us = {q['composed'][0] / q['fused'][0]:.0f}x; "
            f"per-query loop {q['looped'][0] / 1e3:.0f} [{q['looped'][1] / 1e3:.0f} .. {q['looped'][2] / 1e3:.0f}] ms = "
            f"{q['looped'][0] / q['fused'][0]:.0f}x")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
