#!/usr/bin/env python3
"""Timing, memory and accuracy of the fused transformer rows (bt_rows_linear through batrack_amd.frontend.update_former:
rows_linear, forward_rows) -> profiles/r31_update_former_rows.txt.

The tracker's shape: S = 12 frames, N = 1536 and 2400 tracks, hidden 384, 8 heads of 48, MLP 1536, input 456, output 130,
6 time + 6 space blocks.  Two formulations on the same GPU, alternating in one process, warmed up, on the same values:
  rows     one bt_rows_linear launch at "f16x3" and at "f16";
  torch    the statements it replaces as torch operations (F.layer_norm, F.linear, F.gelu, the residual add).
Each of the six Linear shapes with what stands around it in a block, then `forward_rows` at both precisions beside
`update_former.forward`.  Device time between two events (median and 10 % / 90 % quantiles), TFLOP/s counted as float32 FLOP
(2 rows K Nout), the peak memory a call adds beyond its inputs, the largest difference between the routes, and — at
N = 1536, on 4096 sampled rows — each route's error against the statement in float64 as a multiple of torch's.

    python tools/gpu_rows_bench.py [--reps 30] [--out profiles/r31_update_former_rows.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import update_former_util as U  # noqa: E402
from batrack_amd.frontend import update_former  # noqa: E402

DEV = "cuda:0"
S, TRACKS = 12, (1536, 2400)
HIDDEN, HEADS, MLP, INPUT_DIM, OUTPUT_DIM, DEPTH = 384, 8, 1536, 456, 130, 6
EPS = 1e-6
# (name, K, Nout, LayerNorm, GELU, residual): the six Linears of a forward with what one launch fuses around each
LINEARS = (("input_transform", INPUT_DIM, HIDDEN, False, False, False), ("qkv = LN(x) W + b", HIDDEN, 3 * HIDDEN, True, False, False),
           ("x + proj(a)", HIDDEN, HIDDEN, False, False, True), ("GELU(LN(x) W1 + b)", HIDDEN, MLP, True, True, False),
           ("x + fc2(h)", MLP, HIDDEN, False, False, True), ("flow_head", HIDDEN, OUTPUT_DIM, False, False, False))


def alternating(fns, reps, warmup=3):
    """Device times [len(fns), reps] in us, the formulations taking turns."""
    dev = [[] for __ in fns]
    for r in range(reps + warmup):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            dev[i].append(a.elapsed_time(b) * 1e3)
    return np.array(dev)[:, warmup:]


def band(t):
    return f"{np.median(t):9.1f} us [{np.quantile(t, 0.1):8.1f}, {np.quantile(t, 0.9):8.1f}]"


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


def statement(x, lin, ln, gelu, res):
    a = F.layer_norm(x, (x.shape[-1],), None, None, EPS) if ln else x
    v = F.linear(a, lin.weight.to(x.dtype), lin.bias.to(x.dtype))
    if gelu:
        v = F.gelu(v, approximate="tanh")
    return v if res is None else res + v


def model(seed):
    """An UpdateFormer-shaped module tree of the tracker's sizes with seeded weights (update_former_util's attribute names)."""
    g = torch.Generator().manual_seed(seed)

    def lin(fo, fi):
        m = nn.Linear(fi, fo)
        m.weight.data.copy_(torch.randn(fo, fi, generator=g) / fi ** 0.5)
        m.bias.data.copy_(0.1 * torch.randn(fo, generator=g))
        return m

    def block():
        attn = U.Tree(qkv=lin(3 * HIDDEN, HIDDEN), proj=lin(HIDDEN, HIDDEN), q_norm=nn.Identity(), k_norm=nn.Identity(),
                      attn_drop=nn.Dropout(0.0), proj_drop=nn.Dropout(0.0))
        attn.num_heads, attn.scale = HEADS, (HIDDEN // HEADS) ** -0.5
        mlp = U.Tree(fc1=lin(MLP, HIDDEN), act=nn.GELU(approximate="tanh"), drop1=nn.Dropout(0.0), fc2=lin(HIDDEN, MLP), drop2=nn.Dropout(0.0))
        return U.Tree(norm1=nn.LayerNorm(HIDDEN, elementwise_affine=False, eps=EPS), attn=attn,
                      norm2=nn.LayerNorm(HIDDEN, elementwise_affine=False, eps=EPS), mlp=mlp)
    m = U.Tree(input_transform=lin(HIDDEN, INPUT_DIM), flow_head=lin(OUTPUT_DIM, HIDDEN),
               time_blocks=nn.ModuleList([block() for __ in range(DEPTH)]), space_blocks=nn.ModuleList([block() for __ in range(DEPTH)]))
    m.add_space_attn = True
    return m.eval().to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_update_former_rows.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/gpu_rows_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; --reps {args.reps}; all figures measured in this run")
    say("# device time between two events, median [10 %, 90 %], the formulations alternating; TFLOP/s = 2 rows K Nout / median, float32 FLOP")
    net = model(31)
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for N in TRACKS:
            rows = N * S
            say()
            say(f"## one launch against the torch statements it replaces: rows = N S = {N} x {S} = {rows}")
            say(f"{'':24s} {'K':>5s} {'Nout':>5s}  {'torch':>32s} {'f16x3':>32s} {'f16':>32s}  TF/s torch f16x3 f16   x faster f16x3 f16   max |f16x3 - torch|")
            blk = net.time_blocks[0]
            lins = dict(zip([l[0] for l in LINEARS], (net.input_transform, blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2, net.flow_head)))
            for name, K, Nout, ln, gelu, has_res in LINEARS:
                x = (1.5 * torch.randn(rows, K, generator=g) + 0.3).to(DEV)
                res = torch.randn(rows, Nout, generator=g).to(DEV) if has_res else None
                lin = lins[name]
                kw = dict(norm_eps=EPS if ln else None, gelu=gelu, residual=res)
                fns = (lambda: statement(x, lin, ln, gelu, res), lambda: update_former.rows_linear(x, lin, precision="f16x3", **kw),
                       lambda: update_former.rows_linear(x, lin, precision="f16", **kw))
                t = alternating(fns, args.reps)
                med = np.median(t, axis=1)
                tf = 2.0 * rows * K * Nout / med * 1e-6
                diff = float((fns[1]() - fns[0]()).abs().max())
                say(f"{name:24s} {K:5d} {Nout:5d}  {band(t[0])} {band(t[1])} {band(t[2])}  {tf[0]:6.1f} {tf[1]:6.1f} {tf[2]:6.1f}   "
                    f"{med[0] / med[1]:5.2f} {med[0] / med[2]:5.2f}   {diff:.3e}")
                if N == TRACKS[0]:                                  # accuracy on sampled rows: float64 on the GPU
                    idx = torch.randperm(rows, generator=g)[:4096].to(DEV)
                    xs, rs = x[idx].contiguous(), None if res is None else res[idx].contiguous()
                    truth = statement(xs.double(), lin, ln, gelu, None if rs is None else rs.double())
                    e = [float((f.double() - truth).abs().max()) for f in (
                        statement(xs, lin, ln, gelu, rs), update_former.rows_linear(xs, lin, precision="f16x3", norm_eps=kw["norm_eps"], gelu=gelu, residual=rs),
                        update_former.rows_linear(xs, lin, precision="f16", norm_eps=kw["norm_eps"], gelu=gelu, residual=rs))]
                    say(f"{'':24s} error against float64 on 4096 rows: torch {e[0]:.3e}, f16x3 {e[1]:.3e} = {e[1] / e[0]:.2f} x torch's, "
                        f"f16 {e[2]:.3e} = {e[2] / e[0]:.0f} x")
            say()
            say(f"## the whole transformer, {DEPTH} + {DEPTH} blocks, N = {N}, S = {S}: update_former.forward against forward_rows")
            xin = torch.randn(1, N, S, INPUT_DIM, generator=g).to(DEV)
            fns = (lambda: update_former.forward(net, xin), lambda: update_former.forward_rows(net, xin, "f16x3"),
                   lambda: update_former.forward_rows(net, xin, "f16"))
            t = alternating(fns, max(5, args.reps // 3))
            med = np.median(t, axis=1)
            outs = [f() for f in fns]
            for i, name in enumerate(("forward (torch rows)", "forward_rows f16x3", "forward_rows f16")):
                say(f"{name:24s} {band(t[i])}   {med[0] / med[i]:5.2f} x forward   peak added memory {added_memory(fns[i]) / 2 ** 20:8.1f} MiB"
                    + ("" if i == 0 else f"   max |. - forward| {float((outs[i] - outs[0]).abs().max()):.3e} (max |forward| {float(outs[0].abs().max()):.2f})"))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
