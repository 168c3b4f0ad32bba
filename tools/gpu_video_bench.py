#!/usr/bin/env python3
"""Timing and memory of the tracker's input preparation (bt_frame_prep through batrack_amd.frontend.video.prepare_frames) and
of the per-frame cache in front of a tracker call (video.WindowFrames) -> profiles/r30_video_prep.txt.

(a) prepare_frames on 12 and 2 frames of 480 x 854 and 436 x 1024 -> 384 x 512, uint8 HWC and float32 CHW images, beside the
    reference's statements as torch operations on the same GPU (main/batrack.py:668-671, :537-539, md_tracker.py:435-443):
    stack, cat, F.interpolate(bilinear), the in-place colour mapping and the masked min / max.  Alternating in one process,
    warmed up; device time between two events (median, 10 % / 90 % quantiles); the bytes each side must move at the least and
    the rate that makes of our time; the peak memory a call adds beyond its inputs; max |ours - torch|.
(b) the front of a steady-state tracker call at S = 12, kf_stride = 2: on one side two frames pushed into a WindowFrames and
    its window() (prepare 2, encode 2); on the other `prepare_frames(normalise=False)` of all 12, `tracker.forward`'s colour
    mapping and depth range, and the encoder on all 12.  What follows in both (window_depth and embed_conv over the S frames,
    the same calls on the same values) is left out.  Once with `encoder.forward` as the encoder and once with the all-kernel
    encoder (encoder_stem -> encoder_trunk -> encoder_head), on a seeded encoder of the reference's shape.

    python tools/gpu_video_bench.py [--reps 20] [--out profiles/r30_video_prep.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

import encoder_trunk_util as T  # noqa: E402
from batrack_amd.frontend import encoder, tracker, video  # noqa: E402

DEV = "cuda:0"
SIZE, S, SLIDE = (384, 512), 12, 2
SHAPES = ((480, 854), (436, 1024))


def timed(fn, reps, warmup=3):
    dev = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            dev.append(a.elapsed_time(b) * 1e3)
    return np.median(dev), np.quantile(dev, 0.1), np.quantile(dev, 0.9)


def peak_added(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 1e6


def fmt(t):
    return f"{t[0]:.0f} [{t[1]:.0f} .. {t[2]:.0f}] us"


def torch_prepare(images, depths):
    """The reference's statements: the window's lists stacked, colour and depth concatenated, resized, mapped, ranged."""
    rgbs = torch.stack(images, 0)
    dmaps = torch.stack(depths, 0)
    rgbds = torch.cat([rgbs, dmaps[:, None]], 1).float()
    rgbds = Fn.interpolate(rgbds, SIZE, mode="bilinear")
    rgbds[:, :3] = 2 * (rgbds[:, :3] / 255.0) - 1.0
    d = rgbds[:, 3]
    sel = d[d > 0.01]
    return rgbds, torch.stack([sel.min(), sel.max()])


def part_a(reps, lines):
    g = torch.Generator().manual_seed(3)
    for H, W in SHAPES:
        for F in (S, SLIDE):
            for kind in ("uint8 HWC", "float32 CHW"):
                hwc = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
                image = hwc.permute(0, 3, 1, 2) if kind == "uint8 HWC" else hwc.permute(0, 3, 1, 2).float().contiguous()
                depth = (torch.rand(F, H, W, generator=g) * 19.5 + 0.5).to(DEV)
                images, depths = list(image.unbind(0)), list(depth.unbind(0))
                ours = lambda: video.prepare_frames(image, depth, SIZE, True)
                theirs = lambda: torch_prepare(images, depths)
                a, b = ours(), theirs()
                diff = float((a[0] - b[0]).abs().max())
                t_new, t_old = timed(ours, reps), timed(theirs, reps)
                t_new2, t_old2 = timed(ours, reps), timed(theirs, reps)                # alternating: the second pass is quoted
                in_bytes = F * H * W * (3 * (1 if kind == "uint8 HWC" else 4) + 4)
                out_bytes = F * 4 * SIZE[0] * SIZE[1] * 4
                gbs = (in_bytes + out_bytes) / t_new2[0] / 1e3
                lines.append(f"{H} x {W}, {F} frames, {kind}: ours {fmt(t_new2)} (first pass {t_new[0]:.0f}), torch {fmt(t_old2)} (first pass {t_old[0]:.0f}) = "
                             f"{t_old2[0] / t_new2[0]:.2f}x; least traffic {in_bytes / 1e6:.1f} MB read + {out_bytes / 1e6:.1f} MB written = {gbs:.0f} GB/s at our time; "
                             f"peak memory added: ours {peak_added(ours):.1f} MB, torch {peak_added(theirs):.1f} MB; max |ours - torch| {diff:.2e} "
                             f"(colours in [-1, 1], depth to 20: torch's float32 source coordinate)")
                print(lines[-1], flush=True)


def part_b(reps, lines):
    m = T.TrunkEncoder().to(DEV)
    H, W = SHAPES[0]
    g = torch.Generator().manual_seed(5)
    n = S + SLIDE * (reps + 8)
    hwc = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    image = hwc.permute(0, 3, 1, 2)
    depth = (torch.rand(n, H, W, generator=g) * 19.5 + 0.5).to(DEV)
    stride = int(m.stride)

    def all_kernel(x):
        with torch.no_grad():
            maps = encoder.encoder_trunk(encoder.encoder_stem(x, m.conv1), m.layer1, m.layer2, m.layer3, m.layer4)
            return encoder.encoder_head(*maps, m.conv2, m.conv3, (x.shape[2] // stride, x.shape[3] // stride))

    for name, fnet in (("encoder.forward (layer3, layer4 torch)", lambda x: encoder.forward(m, x)), ("all-kernel encoder", all_kernel)):
        wf = video.WindowFrames(S, fnet, size=SIZE)
        for f in range(S):
            wf.push(image[f], depth[f])
        wf.window()
        pos = [S]

        def cached():
            for f in range(pos[0], pos[0] + SLIDE):
                wf.push(image[f], depth[f])
            pos[0] += SLIDE
            return wf.window()

        def plain():
            lo = pos[0] - S
            rgbd, __ = video.prepare_frames(image[lo: pos[0]], depth[lo: pos[0]], SIZE, normalise=False)
            rgbd[:, :3] = 2 * tracker._div_rn(rgbd[:, :3], 255.0) - 1.0
            dr = tracker.depth_range(rgbd[:, 3], False)
            return rgbd, fnet(rgbd[:, :3]), dr

        a, b = cached(), plain()
        same = torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        maps_diff = float((a[1] - b[1]).abs().max())
        t_c, t_p = timed(cached, reps, warmup=3), timed(plain, reps, warmup=3)
        two = timed(lambda: fnet(b[0][:SLIDE, :3]), reps)
        twelve = timed(lambda: fnet(b[0][:, :3]), reps)
        lines.append(f"{name}, {H} x {W} uint8 HWC, S = {S}, slide {SLIDE}: cached front (push {SLIDE}, window()) {fmt(t_c)}; uncached front (prepare {S}, "
                     f"colour mapping, depth range, encode {S}) {fmt(t_p)} = {t_p[0] / t_c[0]:.2f}x; the encoder alone on {SLIDE} frames {fmt(two)}, on {S} {fmt(twelve)}; "
                     f"rgbd and range bit-equal: {same}; max |cached maps - uncached maps| {maps_diff:.2e}; the cache holds "
                     f"{2 * S * (4 * SIZE[0] * SIZE[1] + 128 * (SIZE[0] // stride) * (SIZE[1] // stride)) * 4 / 1e6:.0f} MB")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_video_prep.txt"))
    args = ap.parse_args()
    lines = [f"tracker input on {torch.cuda.get_device_name(0)}: video.prepare_frames (one launch) against the reference's statements as torch operations; "
             f"-> {SIZE[0]} x {SIZE[1]}; alternating, {args.reps} calls each after warm-up; device time between two events, us median [10 % .. 90 %]",
             "(a) prepare_frames(normalise=True): resize, colour mapping, per-frame depth range"]
    part_a(args.reps, lines)
    lines.append("(b) the front of a steady-state tracker call; what both sides share after it (window_depth, embed_conv over the S frames) is left out")
    part_b(args.reps, lines)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(args.out)


if __name__ == "__main__":
    main()
