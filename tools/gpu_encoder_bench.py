#!/usr/bin/env python3
"""Timing and memory of the encoder's head (bt_encoder_head through batrack_amd.frontend.encoder.encoder_head)
-> profiles/r22_encoder_head.txt.

The tracker's shape: a 384 x 512 image at stride 4, so a 96 x 128 output from 192 x 256, 96 x 128, 48 x 64 and 24 x 32 maps of
64, 96, 128 and 128 channels; a full window (S = 12 frames) and a slide (6).  Two formulations on the same GPU, alternating
in one process, warmed up, on the same values:
  new      encoder_head: two launches; the resized copies and the concatenation are never in memory;
  torch    the reference's statements as torch operations (tests/encoder_head_util.head: four F.interpolate, cat, conv2d,
           instance_norm, relu, conv2d).
Device time between two events (median and 10 % / 90 % quantiles), the peak memory a call adds beyond its inputs and its
output, the largest difference between the two results and each one's error against the statements in float64 (frame 0), and — from torch's profiler, where it reports device kernels — the
time of k_head_conv alone and its TFLOP/s (2 x 416 x 9 x 256 FLOP a pixel) against the 155 TFLOP/s float32 MFMA rate.

    python tools/gpu_encoder_bench.py [--reps 30] [--out profiles/r22_encoder_head.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import encoder_head_util as U  # noqa: E402
from batrack_amd.frontend import encoder  # noqa: E402

DEV = "cuda:0"
SIZE, SIZES = (96, 128), ((192, 256), (96, 128), (48, 64), (24, 32))
SHAPES = (("window, S = 12", 12), ("slide, 6 frames", 6))
MFMA_F32_TFLOPS = 155.0
CONV2_FLOP_PER_PIXEL = 2 * U.CIN * 9 * U.CMID


def timed(fn, reps, warmup=3):
    dev = []
    for r in range(reps + warmup):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        dev.append(a.elapsed_time(b) * 1e3)
    return np.array(dev[warmup:])


def added_memory(fn):
    """Peak bytes the call allocates on top of what is live before it, its result included."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def kernel_times(fn, reps):
    """{kernel name: median device time in us} of the project's two kernels, from torch's profiler; {} where it reports none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for r in range(reps):
                fn()
            torch.cuda.synchronize()
        per = {}
        for ev in prof.events():
            for name in ("k_head_conv", "k_head_norm_conv"):
                if name in ev.name:                               # (neither name contains the other)
                    dur = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
                    if dur:
                        per.setdefault(name, []).append(float(dur))
                    break
        return {k: float(np.median(v)) for k, v in per.items()}
    except Exception as e:                                       # a measurement that is missing is reported as missing
        print(f"(profiler unavailable: {e})")
        return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_encoder_head.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is measured without one")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"encoder head on {torch.cuda.get_device_name(0)}: encoder_head (new, two launches) against the reference's statements as torch operations (torch)")
    out(f"{SIZE[0]} x {SIZE[1]} output from " + ", ".join(f"{h} x {w}" for h, w in SIZES) + f" maps; the two alternating, {args.reps} calls each; "
        "us median [10 % .. 90 %]")
    q = lambda v: "{:.0f} [{:.0f} .. {:.0f}]".format(*np.quantile(v, [0.5, 0.1, 0.9]))
    mb = lambda b: f"{b / 1e6:.1f} MB"
    for name, F in SHAPES:
        t = U.random_tensors(100 + F, F, SIZES, device=DEV)
        conv2, conv3 = U.convs(t)
        levels = [t[n] for n in U.NAMES]
        new = lambda: encoder.encoder_head(*levels, conv2, conv3, SIZE)
        with torch.no_grad():
            ref = lambda: U.head(*(t[n] for n in U.INPUTS), SIZE)
            got, want = new(), ref()
            diff = float((got - want).abs().max())
            want64 = U.head(*(t[n][:1].double() for n in U.NAMES), *(t[n].double() for n in U.INPUTS[4:]), SIZE)     # frame 0: frames are independent
            e_new, e_ref = (float((v[:1].double() - want64).abs().max()) for v in (got, want))
            del want64
            d = {"new": [], "torch": []}
            for r in range(2):                                   # alternate the two formulations
                for f, fn in (("new", new), ("torch", ref)):
                    d[f].append(timed(fn, args.reps // 2))
            d = {f: np.concatenate(v) for f, v in d.items()}
            mem = {f: added_memory(fn) for f, fn in (("new", new), ("torch", ref))}
        kt = kernel_times(new, 5)
        flop = CONV2_FLOP_PER_PIXEL * SIZE[0] * SIZE[1] * F
        out(f"{name}: output {mb(got.numel() * 4)}; max |new - torch| {diff:.3e} (max |torch| {float(want.abs().max()):.2f}); "
            f"frame 0 against the statements in float64: new {e_new:.3e}, torch {e_ref:.3e}")
        out(f"  device (events): new {q(d['new'])} us, torch {q(d['torch'])} us = {np.median(d['torch']) / np.median(d['new']):.2f}x")
        out(f"  peak memory a call adds, its output included: new {mb(mem['new'])}, torch {mb(mem['torch'])}"
            f" (the concatenation alone would be {mb(F * U.CIN * SIZE[0] * SIZE[1] * 4)})")
        whole = flop / (np.median(d["new"]) * 1e-6) / 1e12
        if "k_head_conv" in kt:
            tf = flop / (kt["k_head_conv"] * 1e-6) / 1e12
            out(f"  kernels (profiler, median of 5): k_head_conv {kt['k_head_conv']:.0f} us = {tf:.1f} TFLOP/s, {100 * tf / MFMA_F32_TFLOPS:.0f} % of the "
                f"{MFMA_F32_TFLOPS:.0f} TFLOP/s float32 MFMA rate; k_head_norm_conv {kt.get('k_head_norm_conv', float('nan')):.0f} us")
        else:
            out("  kernels: the profiler reported no device kernels: k_head_conv alone is NOT measured")
        out(f"  conv2's {flop / 1e9:.1f} GFLOP over the whole call's device time: {whole:.1f} TFLOP/s (a lower bound for k_head_conv)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
