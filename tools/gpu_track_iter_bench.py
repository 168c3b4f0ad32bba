#!/usr/bin/env python3
"""Timing of the tracker iteration's glue around the update transformers (bt_track_pos_embed, bt_track_tokens,
bt_track_apply through batrack_amd.frontend.track_iter) -> profiles/r18_track_iter.txt.

S = 12 frames, N = 1536 (Sintel) and 2400 (DAVIS) tracks, 96 x 128 maps, tokens of 456 floats.  Two formulations on the
same GPU, alternating in one process, warmed up, on the same inputs:
  new      the kernels: one launch each;
  torch    the torch-operation form of tests/track_iter_util.py, which is how the reference states the loop
           (md_tracker.py:49-61, :249-322): for the position embedding the whole 96 x 128 x 456 table built in numpy float64
           on the host, uploaded and sampled; for the tokens the embedding, the linear layer, the permutes, the cats and
           the two adds; for the state update the slices, group norm, linear layer, GELU, residual, permute and scaling.
Host wall time around a synchronise (what a window pays) and device time between two events, median and 10 % / 90 %
quantiles; the peak device memory a call adds; and the largest difference between the two formulations' results.

    python tools/gpu_track_iter_bench.py [--reps 40] [--out profiles/r18_track_iter.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import track_iter_util as U  # noqa: E402
from batrack_amd.frontend import track_iter as ti  # noqa: E402

DEV = "cuda:0"
S, H, W = 12, 96, 128
SHAPES = (("Sintel", 1536), ("DAVIS", 2400))
SCALE = dict(stride=4.0, Dz=128.0, d_range=19.5, d_near=0.5, use_log_depth=False)


def inputs(N, seed=9):
    g = torch.Generator(device=DEV).manual_seed(seed + N)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    start = torch.rand(1, N, 3, device=DEV, generator=g) * torch.tensor([W - 1.0, H - 1.0, float(W)], device=DEV)
    coords = (start + 2.0 * r(S, N, 3) * (torch.arange(S, device=DEV) > 0)[:, None, None]).contiguous()
    d = dict(coords=coords, fcorrs=r(S, N, U.LRR), ffeats=r(S, N, U.C), track_mask=(r(S, N) > 0).float(), vis=r(S, N) * 4,
             time=ti.time_table(S, U.E, DEV), w_flow=(torch.rand(U.F, U.EMB, device=DEV, generator=g) - 0.5) / 7, b_flow=r(U.F) / 14,
             delta=torch.cat([r(N, S, 3) * 0.5, r(N, S, U.C)], -1).contiguous(), gamma=1 + 0.1 * r(U.C), beta=0.1 * r(U.C),
             w_u=(torch.rand(U.C, U.C, device=DEV, generator=g) - 0.5) / 5.6, b_u=r(U.C) / 11)
    d["pos"] = ti.pos_embed_rows(H, W, U.E, coords[0])
    return d


def calls(d):
    """name -> (new, torch): callables on the same inputs.  The applies work on copies of the state made outside the
    timed region by `prepare`."""
    tok_args = (d["coords"], None, d["fcorrs"], d["ffeats"], d["track_mask"], d["vis"], d["pos"], d["time"], d["w_flow"], d["b_flow"], 0)
    par = (d["gamma"], d["beta"], d["w_u"], d["b_u"])
    state = {}

    def prepare():
        state["c"], state["f"] = d["coords"].clone(), d["ffeats"].clone()

    def apply_new():
        return ti.apply_delta(d["delta"], *par, state["c"], state["f"], **SCALE), state["c"], state["f"]

    def apply_torch():
        c, f, out = U.apply(d["delta"], *par, state["c"], state["f"], **SCALE)
        return out, c.contiguous(), f.contiguous()            # the state back in the layout the lookup wants, as the loop needs it
    return prepare, {
        "sample_pos_embed": (lambda: ti.pos_embed_rows(H, W, U.E, d["coords"][0]), lambda: U.pos_embed_full_table(H, W, U.E, d["coords"][0])),
        "token build": (lambda: ti.build_tokens(*tok_args), lambda: U.tokens(*tok_args)),
        "apply": (apply_new, apply_torch)}


def timed(fn, prepare, reps, warmup=4):
    wall, dev, peak = [], [], 0
    for r in range(reps + warmup):
        prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        tic = time.perf_counter()
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - tic) * 1e6)
        dev.append(a.elapsed_time(b) * 1e3)
        peak = max(peak, torch.cuda.max_memory_allocated() - before)
        del res
    return np.array(wall[warmup:]), np.array(dev[warmup:]), peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_track_iter.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is measured without one")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"tracker iteration glue on {torch.cuda.get_device_name(0)}: the kernels (new) against the torch-operation form (torch)")
    out(f"S = {S}, {H} x {W} maps, tokens of {U.E} floats; the two alternating, {args.reps} calls each; us median [10 % .. 90 %]")
    q = lambda v: "{:.0f} [{:.0f} .. {:.0f}]".format(*np.quantile(v, [0.5, 0.1, 0.9]))
    for name, N in SHAPES:
        d = inputs(N)
        prepare, table = calls(d)
        out(f"{name}: N = {N}, {N * S} tokens, x is {N * S * U.E * 4 / 1e6:.1f} MB")
        for what, (new, old) in table.items():
            prepare()
            rn = new()
            rn = [t.clone() for t in (rn if isinstance(rn, tuple) else (rn,))]
            prepare()
            ro = old()
            ro = ro if isinstance(ro, tuple) else (ro,)
            diff = max(float((a.double() - b.double()).abs().max()) for a, b in zip(rn, ro))
            del rn, ro
            t = {}
            for r in range(2):                                   # alternate the two formulations
                for f, fn in (("new", new), ("torch", old)):
                    w, dv, pk = timed(fn, prepare, args.reps // 2)
                    t.setdefault(f, ([], [], []))
                    t[f][0].append(w)
                    t[f][1].append(dv)
                    t[f][2].append(pk)
            w = {f: np.concatenate(v[0]) for f, v in t.items()}
            dv = {f: np.concatenate(v[1]) for f, v in t.items()}
            pk = {f: max(v[2]) for f, v in t.items()}
            out(f"  {what}: max |new - torch| {diff:.2e}")
            out(f"    host wall: new {q(w['new'])} us, torch {q(w['torch'])} us = {np.median(w['torch']) / np.median(w['new']):.1f}x")
            out(f"    device (events): new {q(dv['new'])} us, torch {q(dv['torch'])} us = {np.median(dv['torch']) / np.median(dv['new']):.1f}x")
            out(f"    peak memory a call adds: new {pk['new'] / 1e6:.1f} MB, torch {pk['torch'] / 1e6:.1f} MB")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
