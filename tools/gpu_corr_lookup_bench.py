#!/usr/bin/env python3
"""Parity figures and timing of the fused correlation lookup (bt_corr_pyramid / bt_corr_lookup, include/batrack_corr.h)
-> profiles/r11_corr_lookup.txt.

Parity: the figures tests/test_gpu_corr_lookup.py asserts on — per fixture case the kernel's error against the
reference's float64 run beside `gate`, the reference's own float32 error (tests/golden/corr_lookup.npz).

Timing, at the tracker's shapes (S 12, C 128, 96 x 128 maps, 4 levels, radius 3; Sintel N 1,536, DAVIS N 2,400): device
events around one `corr` + `sample` pair, warm-up first; the fused pair in each lane layout, the generic kernel and the
float32 volume formulation in torch (tests/corr_util.volume_lookup on a pyramid built beforehand, as the fused one is)
alternating in one process; median and 10 % / 90 % quantiles.  The pyramid's one-off time; peak memory of both pairs
beside the cap the test derives from the sizes.  Gathered bytes from the shapes: S * N * L * (2r+2)^2 feature rows of
4C bytes, over the time, in TB/s beside the guide's figures for gathered rows of this size (7.4-8.6 TB/s chip-wide).

    python tools/gpu_corr_lookup_bench.py [--reps 40] [--out profiles/r11_corr_lookup.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_corr_lookup_bench.py --trace        (a run of its own)
    python tools/gpu_corr_lookup_bench.py --trace-db DIR/.../*_results.db --out FILE      (appends the kernels' times)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import corr_util  # noqa: E402
from batrack_amd import _lib  # noqa: E402
from batrack_amd.frontend.corr import CorrBlock  # noqa: E402

DEV = "cuda:0"
S, C, H, W, L, R = 12, 128, 96, 128, 4, 3
SHAPES = (("Sintel", 1536), ("DAVIS", 2400))
LAYOUTS = ((0, "lanes across channels (default)"), (1, "lane = position"), (2, "generic kernel"))
KERNELS = {0: "k_corr_lookup<0>", 1: "k_corr_lookup<1>", 2: "k_corr_lookup_any"}
TRACE_CALLS = 23


def gathered_bytes(N):
    return S * N * L * (2 * R + 2) ** 2 * 4 * C


def inputs(N, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed + N)
    fmaps = torch.randn(1, S, C, H, W, device=DEV, generator=g)
    targets = torch.randn(1, S, N, C, device=DEV, generator=g)
    u = torch.rand(1, S, N, 3, device=DEV, generator=g)
    coords3 = torch.stack([u[..., 0] * (W + 15) - 8, u[..., 1] * (H + 15) - 8, u[..., 2]], -1).contiguous()
    return fmaps, targets, coords3


def per_call_us(fns, reps, warmup=5):
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


def pair_fns(N):
    fmaps, targets, coords3 = inputs(N)
    coords = coords3[..., :2]
    blk = CorrBlock(fmaps, num_levels=L, radius=R)
    pyr = corr_util.volume_pyramid(fmaps, L)
    lib = _lib.lib()

    def fused(layout):
        def f():
            lib.bt_config_corr_lookup_layout(layout)
            blk.corr(targets)
            return blk.sample(coords)
        return f
    fns = {f"fused {layout}": fused(layout) for layout, _ in LAYOUTS}
    fns["volume"] = lambda: corr_util.volume_lookup(fmaps, targets, coords, L, R, pyramid=pyr)
    return fmaps, targets, fns


def peak_rise(f):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = f()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


def parity(out):
    D = dict(np.load(corr_util.GOLD))
    out("parity against the reference's float64 run (tests/golden/corr_lookup.npz), max |kernel - ref64| over all entries; "
        "gate = the reference's own float32 run against the same")
    for c in corr_util.CASES:
        fmaps, targets, coords3, spec = corr_util.load_case(c)
        t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=DEV)[None]
        ref = D[f"{c}.ref"].astype(np.float64)
        errs = []
        for layout, _ in (LAYOUTS if (spec["C"], spec["r"]) == (C, R) else LAYOUTS[2:]):
            _lib.lib().bt_config_corr_lookup_layout(layout)
            blk = CorrBlock(t(fmaps), num_levels=spec["L"], radius=spec["r"])
            blk.corr(t(targets))
            got = blk.sample(t(coords3)[..., :2])[0].cpu().numpy().astype(np.float64)
            errs.append(f"layout {layout} {np.abs(got - ref).max():.3e} (exact zeros kept {not got[ref == 0].any()})")
        _lib.lib().bt_config_corr_lookup_layout(0)
        out(f"  case {c} (C {spec['C']}, {spec['H']} x {spec['W']}, L {spec['L']}, r {spec['r']}): gate {float(D[f'gate.{c}']):.3e}; " + "; ".join(errs))


def trace_db(args):
    import sqlite3
    cur = sqlite3.connect(args.trace_db).cursor()
    with open(args.out, "a") as fh:
        fh.write(f"kernel time, rocprofv3 --kernel-trace --stats in a run of its own ({TRACE_CALLS} pairs per shape and layout, the first 3 left out):\n")
        for layout, what in LAYOUTS:
            rows = cur.execute("select end - start from kernels where name like ? order by start", (f"%{KERNELS[layout]}%",)).fetchall()
            for k, (name, N) in enumerate(SHAPES):
                t = np.array([r[0] for r in rows[k * TRACE_CALLS:(k + 1) * TRACE_CALLS]][3:]) / 1e3
                if not len(t):
                    continue
                by = gathered_bytes(N)
                fh.write(f"  {name} N {N}, {what}: {KERNELS[layout]} median {np.median(t):.1f} us (min {t.min():.1f}, max {t.max():.1f}), "
                         f"{len(t)} calls; {by / 1e9:.2f} GB gathered = {by / np.median(t) / 1e6:.2f} TB/s\n")
        for kern, cond in (("k_corr_pyramid", "name like '%k_corr_pyramid%' and name not like '%pool%'"),
                           ("k_corr_pyramid_pool", "name like '%k_corr_pyramid_pool%'")):
            rows = cur.execute(f"select end - start from kernels where {cond} order by start").fetchall()
            if rows:
                t = np.array([r[0] for r in rows]) / 1e3
                fh.write(f"  {kern}: {len(t)} launches, median {np.median(t):.1f} us, sum per pyramid {t.sum() / len(SHAPES):.1f} us\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_corr_lookup.txt"))
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--trace", action="store_true", help=f"{TRACE_CALLS} fused pairs per shape and layout, nothing written: for rocprofv3")
    ap.add_argument("--trace-db", help="append the kernels' times per shape from a rocprofv3 results database, then exit")
    args = ap.parse_args()
    if args.trace_db:
        return trace_db(args)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is measured without one")
    if args.trace:
        for _, N in SHAPES:
            _, _, fns = pair_fns(N)
            for layout, _ in LAYOUTS:
                for _ in range(TRACE_CALLS):
                    fns[f"fused {layout}"]()
            torch.cuda.synchronize()
        return
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"fused correlation lookup on {torch.cuda.get_device_name(0)}; S {S}, C {C}, {H} x {W}, {L} levels, radius {R}")
    if not args.no_parity:
        parity(out)
    out(f"timing: device events around each corr + sample pair, {args.reps} pairs each after 5 warm-up rounds, all variants alternating "
        "in one process; us median [10 % .. 90 %]; TB/s = gathered bytes over the median pair time")
    for name, N in SHAPES:
        fmaps, targets, fns = pair_fns(N)
        t = per_call_us(fns, args.reps)
        q = {k: np.quantile(v, [0.5, 0.1, 0.9]) for k, v in t.items()}
        by = gathered_bytes(N)
        out(f"  {name} N {N}: {by / 1e9:.2f} GB gathered per call (arithmetic); volume formulation (torch, float32) "
            f"{q['volume'][0]:.0f} [{q['volume'][1]:.0f} .. {q['volume'][2]:.0f}] us")
        for layout, what in LAYOUTS:
            v = q[f"fused {layout}"]
            out(f"    fused, {what}: {v[0]:.0f} [{v[1]:.0f} .. {v[2]:.0f}] us = {by / v[0] / 1e6:.2f} TB/s; volume / fused {q['volume'][0] / v[0]:.1f}x")
        _lib.lib().bt_config_corr_lookup_layout(0)
        cap = S * N * L * 49 * 4 + targets.numel() * 4 + S * N * 2 * 4 + (1 << 20)
        out(f"    peak memory above the inputs: fused pair {peak_rise(fns['fused 0']) / 1e6:.1f} MB (cap from the sizes {cap / 1e6:.1f} MB), "
            f"volume formulation {peak_rise(fns['volume']) / 1e6:.1f} MB")
        tp = per_call_us({"pyramid": lambda: CorrBlock(fmaps, num_levels=L, radius=R)}, 10, warmup=2)["pyramid"]
        out(f"    pyramid, once per block ({_lib.lib().bt_corr_pyramid_bytes(S, C, H, W, L) / 1e6:.1f} MB written): {np.median(tp):.0f} us")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
