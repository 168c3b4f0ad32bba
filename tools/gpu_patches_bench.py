#!/usr/bin/env python3
"""Timing of the admission of a new frame (bt_image_gradient -> bt_patch_generate through
batrack_amd.frontend.patches.generate_patches) -> profiles/r17_patches.txt.

One frame at 480x854 and at 436x1024, uint8 HWC image as the pipeline hands it over (a permuted view), `grid_grad_20`,
400 patches.  Two formulations on the same GPU, alternating in one process, warmed up, on the same draws:
  new      generate_patches: two launches, the rows of patches_ / colors_ written in place, no host read;
  torch    the statements of the reference in torch operations on the device (main/batrack.py:214-221, :280-325, :917-934
           as restated in tests/patches_util.py: pad, sum, sqrt, avg_pool2d, grid_sample, argsort, gather, the two
           patchify blends, bilinear_sample2d, the uint8 conversion).
Host wall time around a synchronise (what a frame pays) and device time between two events, median and 10 % / 90 %
quantiles.  Also whether the two select the same candidates (they may differ where scores tie: torch's argsort on the
device is not stable) and whether the rows at the device's selection are equal bit for bit.

    python tools/gpu_patches_bench.py [--reps 50] [--out profiles/r17_patches.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import patches_util as pu  # noqa: E402
from batrack_amd.frontend.patches import PatchGenConfig, generate_patches  # noqa: E402

DEV = "cuda:0"
SHAPES = (("DAVIS", 480, 854), ("Sintel", 436, 1024))
G, M = 20, 400


def torch_call(image, depth, ux, uy, patches_row, colors_row):
    H, W = depth.shape
    pad = F.pad(image[None, None], (1, 1, 1, 1), "constant", 0)
    gray = pad.sum(dim=2)
    dx = gray[..., :-1, 1:] - gray[..., :-1, :-1]
    dy = gray[..., 1:, :-1] - gray[..., :-1, :-1]
    g = F.avg_pool2d(torch.sqrt(dx ** 2 + dy ** 2), 4, 4)
    xg, yg = pu.candidates(ux, uy, G, H, W)
    sel = torch.argsort(pu.scores(g[0, 0], xg, yg, H, W), dim=-1)[:, -1:].reshape(-1)
    patches, clr, colors, coords = pu.patch_rows_t(image.float(), depth, xg, yg, sel, 1)
    patches_row.view(M, 3).copy_(patches)
    colors_row.copy_(colors)
    return sel, clr


def new_call(image, depth, ux, uy, patches_row, colors_row):
    r = generate_patches(image, depth, PatchGenConfig(f"grid_grad_{G}", M), draws=(ux, uy), out_patches=patches_row, out_colors=colors_row)
    return r.sel, r.clr[0]


def timed(fn, args, reps, warmup=5):
    wall, dev = [], []
    for r in range(reps + warmup):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        tic = time.perf_counter()
        a.record()
        fn(*args)
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - tic) * 1e6)
        dev.append(a.elapsed_time(b) * 1e3)
    return np.array(wall[warmup:]), np.array(dev[warmup:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_patches.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is measured without one")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"admission of a frame on {torch.cuda.get_device_name(0)}: generate_patches (new) against the reference's statements in torch operations (torch)")
    out(f"grid_grad_{G}, {M} patches, uint8 HWC image; the two alternating, {args.reps} calls each; us median [10 % .. 90 %]")
    q = lambda v: "{:.0f} [{:.0f} .. {:.0f}]".format(*np.quantile(v, [0.5, 0.1, 0.9]))
    for name, H, W in SHAPES:
        rng = np.random.default_rng(H)
        blocks = rng.integers(0, 256, (-(-H // 16), -(-W // 16), 3))
        hwc = np.clip(np.kron(blocks, np.ones((16, 16, 1), np.int64))[:H, :W] + rng.integers(-8, 9, (H, W, 3)), 0, 255).astype(np.uint8)
        image = torch.as_tensor(hwc, device=DEV).permute(2, 0, 1)
        depth = torch.as_tensor(rng.uniform(0.5, 8.0, (H, W)).astype(np.float32), device=DEV)
        ux, uy = torch.rand((G * G, 8), device=DEV), torch.rand((G * G, 8), device=DEV)
        rows = {f: (torch.zeros((M, 3, 1, 1), device=DEV), torch.zeros((M, 3), dtype=torch.uint8, device=DEV)) for f in ("new", "torch")}
        sel_n, clr_n = new_call(image, depth, ux, uy, *rows["new"])
        sel_t, clr_t = torch_call(image, depth, ux, uy, *rows["torch"])
        same_sel = int((sel_n.long() == sel_t).sum())
        xg, yg = pu.candidates(ux, uy, G, H, W)
        at = pu.patch_rows_t(image.float(), depth, xg, yg, sel_n, 1)
        same_rows = torch.equal(at[0].view(torch.int32), rows["new"][0].view(M, 3).view(torch.int32)) and torch.equal(at[2], rows["new"][1])
        t = {}
        for r in range(2):                                       # alternate the two formulations
            for f, fn in (("new", new_call), ("torch", torch_call)):
                w, d = timed(fn, (image, depth, ux, uy, *rows[f]), args.reps // 2)
                t.setdefault(f, ([], []))
                t[f][0].append(w)
                t[f][1].append(d)
        w = {f: np.concatenate(v[0]) for f, v in t.items()}
        d = {f: np.concatenate(v[1]) for f, v in t.items()}
        out(f"{name} {H}x{W}: the two select the same candidate in {same_sel} of {M} cells; the torch statements at the kernel's selection "
            f"give the kernel's rows bit for bit: {same_rows}")
        out(f"  host wall: new {q(w['new'])} us, torch {q(w['torch'])} us = {np.median(w['torch']) / np.median(w['new']):.1f}x")
        out(f"  device (events): new {q(d['new'])} us, torch {q(d['torch'])} us = {np.median(d['torch']) / np.median(d['new']):.1f}x")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
