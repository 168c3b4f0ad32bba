#!/usr/bin/env python3
"""Timing of the tracker's window preparation (bt_depth_range, bt_window_depth, bt_embed_conv, bt_feat_sample through
batrack_amd.frontend.tracker) -> profiles/r21_tracker_window.txt.

96 x 128 maps (384 x 512 images, stride 4), S = 12, a video of 48 frames for the depth range, n = 1536 (Sintel) and 2400
(DAVIS) new tracks; a full window of 12 frames and a slide of 6.  Each kernel beside the reference's statements as torch
operations on the same GPU (md_tracker.py:438-443, :513-517, :519-546, :567-575), alternating in one process, warmed up, on
the same inputs:
  depth range   the boolean-mask compaction, min and max, with their two host reads (the kernel's side reads its pair once);
  window depth  the clone, the normalisation, F.interpolate, the scaling, and the min / max the embedding takes of them;
  convolution   the min-max normalisation, the 21 tensors of `featPE` and their cat, the cat with the encoder's maps and
                F.conv2d — for the slide the torch side builds all 12 frames and convolves 6, as the reference does.
                Achieved TFLOP/s = 2 * 9 * 191 * 128 flop per output pixel, against the 155 TF float32 MFMA rate;
  feat_init     the gather of one whole map per query, its permuted copy, and the four [n, n, C] gathers with their
                diagonals.  Timed at n = 256, and at the larger n only where twice the gather and the four [n, n, C] tensors
                fit in a quarter of the free device memory (the machines are shared).
Device time between two events, median and 10 % / 90 % quantiles; the peak device memory a call adds; the largest
difference between the two formulations' results.

    python tools/gpu_tracker_window_bench.py [--reps 20] [--out profiles/r21_tracker_window.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

import tracker_window_util as U  # noqa: E402
from batrack_amd.frontend import tracker as tw  # noqa: E402

DEV = "cuda:0"
S, T, H, W, STRIDE = 12, 48, 384, 512, 4
h, w = H // STRIDE, W // STRIDE
D_NEAR, D_FAR, DZ = 0.5, 20.0, float(w)
PEAK_TF = 155.0


def torch_depth_range(depth):
    return depth[depth > 0.01].min().item(), depth[depth > 0.01].max().item()


def torch_window_depth(depth):
    d = depth[:, None].clone()
    d = (d - D_NEAR) / (D_FAR - D_NEAR)
    dn = Fn.interpolate(d, scale_factor=1.0 / STRIDE, mode="nearest") * DZ
    return dn[:, 0], torch.stack([dn.min(), dn.max()])


def torch_embed_conv(fnet, dmaps, frame0, conv):
    """All S frames of the embedding are built, as the reference does; frames frame0 .. are convolved."""
    gx = torch.linspace(0, w - 1, w, device=DEV)[None, None, :].expand(S, h, w)
    gy = torch.linspace(0, h - 1, h, device=DEV)[None, :, None].expand(S, h, w)
    g = torch.stack([gx, gy, dmaps], 1).clone()
    for a in range(3):
        g[:, a] = (g[:, a] - g[:, a].min()) / (g[:, a].max() - g[:, a].min())
    g = (2 * (g - 0.5)).permute(0, 2, 3, 1).reshape(S * h * w, 3)
    out = [g]
    for f in U.FREQS:
        out += [torch.sin(g * f), torch.cos(g * f)]
    pe = torch.cat(out, -1).view(S, h, w, -1).permute(0, 3, 1, 2)
    return conv(torch.cat([fnet, pe[frame0:]], 1))


def torch_feat_init(fmaps, frames, xy):
    """md_tracker.py:567-575 with model_utils.py:94-154, five-dimensional branch."""
    n = frames.numel()
    sample = fmaps[None][:, frames.long()]                                   # [1, n, C, h, w]: one whole map per query
    flat = sample.permute(0, 3, 4, 1, 2).reshape(h * w, n, U.C)              # the permuted copy
    x, y = xy[None, :, 0], xy[None, :, 1]
    x0, y0 = torch.floor(x).int(), torch.floor(y).int()
    x1, y1 = x0 + 1, y0 + 1
    cx0, cx1, cy0, cy1 = x0.clamp(0, w - 1), x1.clamp(0, w - 1), y0.clamp(0, h - 1), y1.clamp(0, h - 1)
    tap = lambda cy, cx: torch.diagonal(flat[(cy * w + cx).long()], dim1=1, dim2=2).permute(0, 2, 1)
    out = (((x1.float() - x) * (y1.float() - y)).unsqueeze(2) * tap(cy0, cx0) + ((x - x0.float()) * (y1.float() - y)).unsqueeze(2) * tap(cy0, cx1)
           + ((x1.float() - x) * (y - y0.float())).unsqueeze(2) * tap(cy1, cx0) + ((x - x0.float()) * (y - y0.float())).unsqueeze(2) * tap(cy1, cx1))
    return out[0]


def timed(fns, reps):
    """Device time in microseconds of each callable, alternating; the peak memory each adds."""
    times, peaks = [[] for _ in fns], []
    for f in fns:
        f()
        f()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        f()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            times[i].append(a.elapsed_time(b) * 1e3)
    return [np.percentile(t, [50, 10, 90]) for t in times], peaks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_tracker_window.txt"))
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(21)
    video = torch.rand(1, T, 4, H, W, device=DEV, generator=g) * 19.5 + 0.5
    video[0, :, 3, :4, :4] = 0.0
    depth_all, depth_win = video[0, :, 3], video[0, :S, 3]
    fnet = torch.randn(S, U.C, h, w, device=DEV, generator=g)
    conv = torch.nn.Conv2d(U.C + U.EMB, U.C, 3, padding=1).to(DEV).requires_grad_(False)
    dmaps, zrange = tw.window_depth(depth_win, S, STRIDE, D_NEAR, D_FAR, DZ)
    lines = [f"tracker window preparation on {torch.cuda.get_device_name(0)}: the kernels (new) against the reference's statements as torch operations (torch)",
             f"S = {S}, {h} x {w} maps, a video of {T} frames; the two alternating, {args.reps} calls each; device us median [10 % .. 90 %]"]

    def report(name, new, ref, diff, extra=""):
        (tn, tt), (pn, pt) = timed([new, ref], args.reps)
        lines.append(f"  {name}: max |new - torch| {diff:.2e}{extra}")
        lines.append(f"    device (events): new {tn[0]:.0f} [{tn[1]:.0f} .. {tn[2]:.0f}] us, torch {tt[0]:.0f} [{tt[1]:.0f} .. {tt[2]:.0f}] us = {tt[0] / tn[0]:.1f}x")
        lines.append(f"    peak memory a call adds: new {pn / 1e6:.1f} MB, torch {pt / 1e6:.1f} MB")
        print("\n".join(lines[-3:]), flush=True)
        return tn[0]

    with torch.no_grad():
        a, b = tw.depth_range(depth_all).tolist(), torch_depth_range(depth_all)
        report("depth range (with the host read)", lambda: tw.depth_range(depth_all).tolist(), lambda: torch_depth_range(depth_all),
               max(abs(a[0] - b[0]), abs(a[1] - b[1])))
        report("window depth and its range", lambda: tw.window_depth(depth_win, S, STRIDE, D_NEAR, D_FAR, DZ), lambda: torch_window_depth(depth_win),
               float((dmaps - torch_window_depth(depth_win)[0]).abs().max()))
        for label, frame0 in (("full window, 12 frames", 0), ("slide, 6 frames", S // 2)):
            F = S - frame0
            out = torch.empty(F, U.C, h, w, device=DEV)
            new = lambda: tw.embed_conv(fnet[frame0:], dmaps, zrange, frame0, conv, U.FREQS, out=out)
            ref = lambda: torch_embed_conv(fnet[frame0:], dmaps, frame0, conv)
            diff = float((new() - ref()).abs().max())
            t = report(f"embedding and convolution, {label}", new, ref, diff)
            flop = 2.0 * 9 * (U.C + U.EMB) * U.C * F * h * w
            lines.append(f"    {flop / 1e9:.1f} GFLOP: new {flop / t / 1e6:.1f} TFLOP/s = {100 * flop / t / 1e6 / PEAK_TF:.0f} % of {PEAK_TF:.0f} TF")
            print(lines[-1], flush=True)
        fmaps = tw.embed_conv(fnet, dmaps, zrange, 0, conv, U.FREQS)
        for n in (256, 1536, 2400):
            frames = torch.randint(0, S, (n,), device=DEV, generator=g).to(torch.int32)
            xy = torch.rand(n, 3, device=DEV, generator=g) * torch.tensor([w + 6.0, h + 6.0, 1.0], device=DEV) - 3.0
            new = lambda: tw.sample_features(fmaps, frames, xy)
            need = 2 * n * U.C * h * w * 4 + 4 * n * n * U.C * 4
            free = torch.cuda.mem_get_info()[0]
            if need > free // 4:
                (tn,), (pn,) = timed([new], args.reps)
                lines.append(f"  feat_init, n = {n}: new {tn[0]:.0f} [{tn[1]:.0f} .. {tn[2]:.0f}] us, adds {pn / 1e6:.2f} MB; torch not run: its "
                             f"{need / 1e9:.1f} GB do not fit a quarter of the {free / 1e9:.0f} GB free")
                print(lines[-1], flush=True)
                continue
            diff = float((new() - torch_feat_init(fmaps, frames, xy)).abs().max())
            report(f"feat_init, n = {n}", new, lambda: torch_feat_init(fmaps, frames, xy), diff)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
