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

--trunk measures the encoder's trunk instead (bt_res_block through encoder.residual_block / encoder_trunk)
-> profiles/r26_encoder_trunk.txt: layer1..4 from a 64 x 192 x 256 input, 12 frames and 6, each layer and the whole trunk
beside the same nn.Sequential layers run by torch on the same GPU (what `forward` executes for a layer that is not in
encoder.DEVICE_LAYERS), alternating, device time between two events; the peak memory a call adds; frame 0 of every level
against the statements in float64; `encoder.forward` on a 384 x 512 image with DEVICE_LAYERS as committed and empty (every
layer called as it is); and the list DEVICE_LAYERS must be by the rule "not above torch's time at both shapes".  The kernel
rows come from one rocprofv3 run of its own:

    python tools/gpu_encoder_bench.py --trunk [--reps 20] [--out profiles/r26_encoder_trunk.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_encoder_bench.py --trunk-trace        (a run of its own)
    python tools/gpu_encoder_bench.py --trunk-trace-db DIR/.../*_results.db [--out ...]                  (appends the kernel rows)

--stem measures the encoder's stem (bt_encoder_stem through encoder.encoder_stem) -> profiles/r28_encoder_stem.txt: 12 and 6
frames of 3 x 384 x 512 beside `relu1(norm1(conv1(x)))` with the modules as the reference builds them (the ReLU in place),
alternating, device time between two events; the peak memory a call adds; frame 0 of both against the statements in float64;
`encoder.forward` on the same image with DEVICE_STEM on and off (off is the parent's forward); and the value DEVICE_STEM must
have by the rule "not above torch's time at both shapes".  The kernel rows come from one rocprofv3 run of its own:

    python tools/gpu_encoder_bench.py --stem [--reps 20] [--out profiles/r28_encoder_stem.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_encoder_bench.py --stem-trace          (a run of its own)
    python tools/gpu_encoder_bench.py --stem-trace-db DIR/.../*_results.db [--out ...]                    (appends the kernel rows)
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

# ------------------------------------------------------------------------------------------------------------- the trunk
TRUNK_SIZE, TRUNK_IMAGE = (192, 256), (384, 512)
TRACE_CALLS, TRACE_SKIP = 8, 3
LAUNCHES = ("conv1", "stats1", "conv2", "stats2", "join")       # bt_res_block's five launches, in order


def trunk_setup(F):
    import encoder_trunk_util as T
    t = {k: torch.as_tensor(v, dtype=torch.float32, device=DEV) for k, v in T.make_inputs(200 + F, 1, (2, 2)).items() if "." in k and not k.startswith("in.")}
    layers = T.make_layers(t)
    x = torch.rand(F, 64, *TRUNK_SIZE, generator=torch.Generator(device=DEV).manual_seed(300 + F), device=DEV) * 2.0
    return T, t, layers, x


def block_flops(F):
    """Per block: (conv1, shortcut, conv2) FLOP of F frames from the 192 x 256 input."""
    import encoder_trunk_util as T
    sizes, out = T.level_sizes(TRUNK_SIZE), []
    for layer, i, c_in, c_out, stride in T.BLOCKS:
        ho, wo = sizes[T.LAYERS.index(layer)]
        n = F * ho * wo
        out.append((2 * 9 * c_in * c_out * n, 2 * c_in * c_out * n if stride == 2 else 0, 2 * 9 * c_out * c_out * n))
    return out


def trunk_trace():
    for __, F in SHAPES:
        T, t, layers, x = trunk_setup(F)
        for r in range(TRACE_CALLS):
            encoder.encoder_trunk(x, *layers)
        torch.cuda.synchronize()


def trunk_trace_db(args):
    import sqlite3
    import encoder_trunk_util as T
    cur = sqlite3.connect(args.trunk_trace_db).cursor()
    rows = cur.execute("select name, end - start, vgpr_count, accum_vgpr_count, lds_size from kernels where name like '%k_res_%' or name like '%k_conv_stats%' order by start").fetchall()
    per_call = len(T.BLOCKS) * len(LAUNCHES)
    with open(args.out, "a") as fh:
        fh.write(f"kernel time, rocprofv3 --kernel-trace --stats in a run of its own ({TRACE_CALLS} trunks per shape, the first {TRACE_SKIP} left out): "
                 f"median us; convolutions with their TFLOP/s (the shortcut's products counted with conv1) and share of the {MFMA_F32_TFLOPS:.0f} TFLOP/s "
                 "float32 MFMA rate; LDS as the trace reports it (registers: -Rpass-analysis=kernel-resource-usage, DESIGN.md f-13)\n")
        if len(rows) != len(SHAPES) * TRACE_CALLS * per_call:
            fh.write(f"  ({len(rows)} k_res_* launches in the trace, {len(SHAPES) * TRACE_CALLS * per_call} expected: rows NOT attributed)\n")
            return
        for k, (name, F) in enumerate(SHAPES):
            part = rows[k * TRACE_CALLS * per_call:(k + 1) * TRACE_CALLS * per_call]
            flops, total, mfma = block_flops(F), 0.0, 0.0
            fh.write(f"  {name}:\n")
            for b, (layer, i, c_in, c_out, stride) in enumerate(T.BLOCKS):
                cells = []
                for j, launch in enumerate(LAUNCHES):
                    sel = [part[c * per_call + b * len(LAUNCHES) + j] for c in range(TRACE_SKIP, TRACE_CALLS)]
                    us = float(np.median([r[1] for r in sel])) / 1e3
                    total += us
                    cell = f"{launch} {us:.0f}"
                    if launch in ("conv1", "conv2"):
                        fl = flops[b][0] + flops[b][1] if launch == "conv1" else flops[b][2]
                        tf = fl / (us * 1e-6) / 1e12
                        mfma += us
                        cell += f" ({tf:.1f} TFLOP/s, {100 * tf / MFMA_F32_TFLOPS:.0f} %; {sel[0][4]} B LDS)"
                    cells.append(cell)
                fh.write(f"    {layer}[{i}] {c_in} -> {c_out} stride {stride}: " + ", ".join(cells) + "\n")
            fl = sum(sum(v) for v in flops)
            fh.write(f"    sum of the 40 launches {total:.0f} us, of the 16 convolutions {mfma:.0f} us = {fl / (mfma * 1e-6) / 1e12:.1f} TFLOP/s over {fl / 1e9:.1f} GFLOP\n")


def trunk_main(args):
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    q = lambda v: "{:.0f} [{:.0f} .. {:.0f}]".format(*np.quantile(v, [0.5, 0.1, 0.9]))
    mb = lambda b: f"{b / 1e6:.1f} MB"
    out(f"encoder trunk on {torch.cuda.get_device_name(0)}: layer1..4 on bt_res_block (new) against the same nn.Sequential layers run by torch (torch)")
    out(f"64 x {TRUNK_SIZE[0]} x {TRUNK_SIZE[1]} input; the two alternating, {args.reps} calls each after warm-up; device time between two events, us median [10 % .. 90 %]")
    keep = {}
    for name, F in SHAPES:
        T, t, layers, x = trunk_setup(F)
        with torch.no_grad():
            inputs = [x]
            for layer in layers[:3]:
                inputs.append(layer(inputs[-1]))
            pairs = [(n, (lambda l=l, v=v: encoder._run_layer(v, l)), (lambda l=l, v=v: l(v))) for n, l, v in zip(T.LAYERS, layers, inputs)]

            def torch_trunk():
                v, outs = x, []
                for l in layers:
                    v = l(v)
                    outs.append(v)
                return outs
            pairs.append(("trunk", lambda: encoder.encoder_trunk(x, *layers), torch_trunk))
            got, want = encoder.encoder_trunk(x, *layers), torch_trunk()
            want64 = T.trunk(x[:1].double(), {k: v.double() for k, v in t.items()})               # frame 0: frames are independent
            errs = [(float((g[:1].double() - w64).abs().max()), float((w[:1].double() - w64).abs().max())) for g, w, w64 in zip(got, want, want64)]
            del want64, got, want
            out(f"{name}: frame 0 of a, b, c, d against the statements in float64, max |new - f64| / max |torch - f64|: "
                + ", ".join(f"{a:.2e} / {b:.2e}" for a, b in errs))
            for n, new, ref in pairs:
                d = {"new": [], "torch": []}
                for r in range(2):                                   # alternate the two formulations
                    for f, fn in (("new", new), ("torch", ref)):
                        d[f].append(timed(fn, args.reps // 2))
                d = {f: np.concatenate(v) for f, v in d.items()}
                mem = {f: added_memory(fn) for f, fn in (("new", new), ("torch", ref))}
                keep[n, F] = (float(np.median(d["new"])), float(np.median(d["torch"])))
                fl = sum(sum(v) for v, blk in zip(block_flops(F), T.BLOCKS) if n in ("trunk", blk[0]))
                out(f"  {n}: new {q(d['new'])} us, torch {q(d['torch'])} us = {np.median(d['torch']) / np.median(d['new']):.2f}x; "
                    f"{fl / 1e9:.1f} GFLOP over the call's device time: new {fl / np.median(d['new']) / 1e6:.1f}, torch {fl / np.median(d['torch']) / 1e6:.1f} TFLOP/s; "
                    f"peak memory a call adds, its output included: new {mb(mem['new'])}, torch {mb(mem['torch'])}")
            del pairs, inputs
            m = T.TrunkEncoder().to(DEV)
            img = torch.rand(F, 3, *TRUNK_IMAGE, generator=torch.Generator(device=DEV).manual_seed(400 + F), device=DEV) * 2 - 1
            committed = encoder.DEVICE_LAYERS

            def forward_with(which):
                encoder.DEVICE_LAYERS = which
                try:
                    return encoder.forward(m, img)
                finally:
                    encoder.DEVICE_LAYERS = committed
            d = {"committed": [], "none": []}
            for r in range(2):
                for f, which in (("committed", committed), ("none", ())):
                    d[f].append(timed(lambda: forward_with(which), args.reps // 2))
            d = {f: np.concatenate(v) for f, v in d.items()}
            out(f"  encoder.forward on a {TRUNK_IMAGE[0]} x {TRUNK_IMAGE[1]} image: DEVICE_LAYERS = {committed} {q(d['committed'])} us; "
                f"empty (every layer called as it is, the parent's forward) {q(d['none'])} us = {np.median(d['none']) / np.median(d['committed']):.2f}x")
            del m, img
        torch.cuda.empty_cache()
    rule = tuple(n for n in ("layer1", "layer2", "layer3", "layer4") if all(keep[n, F][0] <= keep[n, F][1] for __, F in SHAPES))
    out(f"DEVICE_LAYERS by the rule (a layer's device time not above torch's at both shapes): {rule}; committed: {encoder.DEVICE_LAYERS}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


# -------------------------------------------------------------------------------------------------------------- the stem
STEM_LAUNCHES = ("k_stem_conv", "k_conv_stats", "k_stem_norm")  # bt_encoder_stem's three launches, in order
STEM_K, STEM_K_PADDED = 147, 168


def stem_setup(F):
    import encoder_stem_util as S
    m = S.StemEncoder(seed=500 + F).to(DEV)
    x = torch.rand(F, 3, *TRUNK_IMAGE, generator=torch.Generator(device=DEV).manual_seed(600 + F), device=DEV) * 2 - 1
    return S, m, x


def stem_flop(F, k=STEM_K):
    return 2 * k * 64 * (TRUNK_IMAGE[0] // 2) * (TRUNK_IMAGE[1] // 2) * F


def stem_trace():
    for __, F in SHAPES:
        S, m, x = stem_setup(F)
        for r in range(TRACE_CALLS):
            encoder.encoder_stem(x, m.conv1)
        torch.cuda.synchronize()


def stem_trace_db(args):
    import sqlite3
    cur = sqlite3.connect(args.stem_trace_db).cursor()
    rows = cur.execute("select name, end - start, vgpr_count, accum_vgpr_count, lds_size from kernels where name like '%k_stem_%' or name like '%k_conv_stats%' order by start").fetchall()
    per_call = len(STEM_LAUNCHES)
    with open(args.out) as fh:
        lines = fh.read().splitlines()
    last = lines.pop()                                           # the rule's outcome stays the last line
    lines.append(f"kernel time, rocprofv3 --kernel-trace --stats in a run of its own ({TRACE_CALLS} stems per shape, the first {TRACE_SKIP} left out): "
                 f"median us; the convolution with its TFLOP/s over the {STEM_K} products a pixel (and over the {STEM_K_PADDED} it multiplies) and share of "
                 f"the {MFMA_F32_TFLOPS:.0f} TFLOP/s float32 MFMA rate; the elementwise pass with its GB/s")
    if len(rows) != len(SHAPES) * TRACE_CALLS * per_call or any(STEM_LAUNCHES[i % per_call] not in r[0] for i, r in enumerate(rows)):
        lines.append(f"  ({len(rows)} k_stem_* launches in the trace, {len(SHAPES) * TRACE_CALLS * per_call} expected: rows NOT attributed)")
    else:
        for k, (name, F) in enumerate(SHAPES):
            part = rows[k * TRACE_CALLS * per_call:(k + 1) * TRACE_CALLS * per_call]
            cells, total = [], 0.0
            for j, launch in enumerate(STEM_LAUNCHES):
                sel = [part[c * per_call + j] for c in range(TRACE_SKIP, TRACE_CALLS)]
                us = float(np.median([r[1] for r in sel])) / 1e3
                total += us
                cell = f"{launch} {us:.0f}"
                if launch == "k_stem_conv":
                    tf, tfp = (stem_flop(F, kk) / (us * 1e-6) / 1e12 for kk in (STEM_K, STEM_K_PADDED))
                    cell += f" ({tf:.1f} TFLOP/s, {100 * tf / MFMA_F32_TFLOPS:.0f} %; padded {tfp:.1f}, {100 * tfp / MFMA_F32_TFLOPS:.0f} %; {sel[0][4]} B LDS)"
                if launch == "k_stem_norm":
                    cell += f" ({2 * stem_flop(F, 1) * 2 / (us * 1e-6) / 1e9:.0f} GB/s read and written)"
                cells.append(cell)
            lines.append(f"  {name}: " + ", ".join(cells) + f"; sum of the three launches {total:.0f} us")
    lines.append(last)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def stem_main(args):
    import encoder_trunk_util as T
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    q = lambda v: "{:.0f} [{:.0f} .. {:.0f}]".format(*np.quantile(v, [0.5, 0.1, 0.9]))
    mb = lambda b: f"{b / 1e6:.1f} MB"
    out(f"encoder stem on {torch.cuda.get_device_name(0)}: encoder_stem (new, three launches) against relu1(norm1(conv1(x))) with the modules as the "
        "reference builds them, the ReLU in place (torch)")
    out(f"3 x {TRUNK_IMAGE[0]} x {TRUNK_IMAGE[1]} images; the two alternating, {args.reps} calls each after warm-up; device time between two events, "
        "us median [10 % .. 90 %]")
    keep = {}
    for name, F in SHAPES:
        S, m, x = stem_setup(F)
        with torch.no_grad():
            new = lambda: encoder.encoder_stem(x, m.conv1)
            ref = lambda: m.relu1(m.norm1(m.conv1(x)))
            got, want = new(), ref()
            want64 = S.stem(x[:1].double(), m.conv1.weight.double(), m.conv1.bias.double())     # frame 0: frames are independent
            e_new, e_ref = (float((v[:1].double() - want64).abs().max()) for v in (got, want))
            diff = float((got - want).abs().max())
            del want64, got, want
            d = {"new": [], "torch": []}
            for r in range(2):                                   # alternate the two formulations
                for f, fn in (("new", new), ("torch", ref)):
                    d[f].append(timed(fn, args.reps // 2))
            d = {f: np.concatenate(v) for f, v in d.items()}
            mem = {f: added_memory(fn) for f, fn in (("new", new), ("torch", ref))}
            keep[F] = (float(np.median(d["new"])), float(np.median(d["torch"])))
            fl = stem_flop(F)
            out(f"{name}: output {mb(F * 64 * (TRUNK_IMAGE[0] // 2) * (TRUNK_IMAGE[1] // 2) * 4)}; max |new - torch| {diff:.3e}; frame 0 against the "
                f"statements in float64: new {e_new:.3e}, torch {e_ref:.3e}")
            out(f"  device (events): new {q(d['new'])} us, torch {q(d['torch'])} us = {np.median(d['torch']) / np.median(d['new']):.2f}x; "
                f"{fl / 1e9:.1f} GFLOP over the call's device time: new {fl / np.median(d['new']) / 1e6:.1f}, torch {fl / np.median(d['torch']) / 1e6:.1f} TFLOP/s")
            out(f"  peak memory a call adds, its output included: new {mb(mem['new'])}, torch {mb(mem['torch'])}")
            enc = T.TrunkEncoder().to(DEV)
            committed = encoder.DEVICE_STEM

            def forward_with(flag):
                encoder.DEVICE_STEM = flag
                try:
                    return encoder.forward(enc, x)
                finally:
                    encoder.DEVICE_STEM = committed
            d = {True: [], False: []}
            for r in range(2):
                for flag in (True, False):
                    d[flag].append(timed(lambda: forward_with(flag), args.reps // 2))
            d = {f: np.concatenate(v) for f, v in d.items()}
            out(f"  encoder.forward on the same images: DEVICE_STEM on {q(d[True])} us; off (conv1, norm1, relu1 called as they are, the parent's "
                f"forward) {q(d[False])} us = {np.median(d[False]) / np.median(d[True]):.2f}x")
            del enc, m, x
        torch.cuda.empty_cache()
    rule = all(keep[F][0] <= keep[F][1] for __, F in SHAPES)
    out(f"DEVICE_STEM by the rule (the stem's device time not above torch's at both shapes): {rule}; committed: {encoder.DEVICE_STEM}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out")
    ap.add_argument("--trunk", action="store_true", help="measure the trunk (layer1..4) instead of the head")
    ap.add_argument("--trunk-trace", action="store_true", help=f"{TRACE_CALLS} trunks per shape, nothing written: for rocprofv3")
    ap.add_argument("--trunk-trace-db", help="append the trunk kernels' rows from a rocprofv3 results database, then exit")
    ap.add_argument("--stem", action="store_true", help="measure the stem (conv1, norm1, relu1) instead of the head")
    ap.add_argument("--stem-trace", action="store_true", help=f"{TRACE_CALLS} stems per shape, nothing written: for rocprofv3")
    ap.add_argument("--stem-trace-db", help="append the stem kernels' rows from a rocprofv3 results database, then exit")
    args = ap.parse_args()
    trunk = args.trunk or args.trunk_trace or args.trunk_trace_db
    stem = args.stem or args.stem_trace or args.stem_trace_db
    args.out = args.out or os.path.join(ROOT, "profiles", "r28_encoder_stem.txt" if stem else "r26_encoder_trunk.txt" if trunk else "r22_encoder_head.txt")
    if args.trunk_trace_db:
        return trunk_trace_db(args)
    if args.stem_trace_db:
        return stem_trace_db(args)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is measured without one")
    if args.stem_trace:
        return stem_trace()
    if args.stem:
        return stem_main(args)
    if args.trunk_trace:
        return trunk_trace()
    if args.trunk:
        return trunk_main(args)
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
