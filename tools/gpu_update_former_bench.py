#!/usr/bin/env python3
"""Timing of the update transformer's attention core (bt_attention through batrack_amd.frontend.update_former) and of one
whole UpdateFormer.forward built on it -> profiles/r19_update_former.txt.

S = 12 frames, N = 1536 (Sintel) and 2400 (DAVIS) tracks, hidden 384, 8 heads of 48, 6 time and 6 space blocks, tokens of
456 floats in, 131 out.  Formulations on the same GPU, alternating in one process, warmed up, on the same inputs:
  new      bt_attention on the qkv Linear's output [N S, 1152] in place: one launch, no copy;
  matmul   what the reference runs (cotracker/blocks.py:441-454 around timm's Attention): for the space axis one copy of the
           activation [N, S, 384] -> [S, N, 384] before the block and one back after it (with B = 1 the rearranges
           themselves are views; the LayerNorm that follows each materialises it), the permute of the qkv output,
           (q * scale) @ k^T, softmax, @ v, and the transpose-reshape copy of the result.  The qkv the torch forms read is
           laid out for them OUTSIDE the timed region;
  sdpa     the same with F.scaled_dot_product_attention in place of matmul-softmax-matmul.
Device time between two events and host wall time around a synchronise, median and 10 % / 90 % quantiles; the peak device
memory a call adds; the largest difference between the formulations' results; and the space kernel's achieved FLOP/s
(4 N^2 48 heads S operations a call, counted from the shapes) against the 155 TF float32 MFMA rate.

    python tools/gpu_update_former_bench.py [--reps 20] [--out profiles/r19_update_former.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import update_former_util as U  # noqa: E402
from batrack_amd.frontend import update_former as uf  # noqa: E402

DEV = "cuda:0"
S, HIDDEN, HEADS, HD, DEPTH, IN_DIM, OUT_DIM = 12, 384, 8, 48, 6, 456, 131
SHAPES = (("Sintel", 1536), ("DAVIS", 2400))
MFMA_F32_PEAK = 155e12


def timm_core(qkv, sdpa):
    """qkv [B, L, 3 C] -> [B, L, C] as timm's Attention does between its two Linears."""
    B, L, __ = qkv.shape
    q, k, v = qkv.reshape(B, L, 3, HEADS, HD).permute(2, 0, 3, 1, 4).unbind(0)
    if sdpa:
        x = F.scaled_dot_product_attention(q, k, v)
    else:
        x = ((q * HD ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1) @ v
    return x.transpose(1, 2).reshape(B, L, HEADS * HD)


def core_calls(N, seed=19):
    g = torch.Generator(device=DEV).manual_seed(seed + N)
    qkv = torch.randn(N * S, 3 * HIDDEN, device=DEV, generator=g)
    x = torch.randn(N, S, HIDDEN, device=DEV, generator=g)                       # stands for the activation the reference rearranges
    qkv_t = qkv.reshape(N, S, 3 * HIDDEN)
    qkv_s = qkv_t.permute(1, 0, 2).contiguous()

    def space_torch(sdpa):
        x_space = x.permute(1, 0, 2).contiguous()                                # "b n t c -> (b t) n c", materialised
        o = timm_core(qkv_s, sdpa)
        del x_space
        return o.permute(1, 0, 2).contiguous().reshape(N * S, HIDDEN)            # and back
    return {
        "time axis": dict(new=lambda: uf.attention(qkv, HEADS, N, S, S, 1),
                          matmul=lambda: timm_core(qkv_t, False).reshape(N * S, HIDDEN),
                          sdpa=lambda: timm_core(qkv_t, True).reshape(N * S, HIDDEN)),
        "space axis": dict(new=lambda: uf.attention(qkv, HEADS, S, N, 1, S), matmul=lambda: space_torch(False), sdpa=lambda: space_torch(True))}


def make_model(seed=23):
    torch.manual_seed(seed)
    lin = lambda i, o: nn.Linear(i, o)

    def blk():
        attn = U.Tree(qkv=lin(HIDDEN, 3 * HIDDEN), proj=lin(HIDDEN, HIDDEN), q_norm=nn.Identity(), k_norm=nn.Identity())
        attn.num_heads, attn.scale = HEADS, HD ** -0.5
        return U.Tree(norm1=nn.LayerNorm(HIDDEN, elementwise_affine=False, eps=1e-6), attn=attn,
                      norm2=nn.LayerNorm(HIDDEN, elementwise_affine=False, eps=1e-6),
                      mlp=U.Tree(fc1=lin(HIDDEN, 4 * HIDDEN), act=nn.GELU(approximate="tanh"), fc2=lin(4 * HIDDEN, HIDDEN)))
    m = U.Tree(input_transform=lin(IN_DIM, HIDDEN), flow_head=lin(HIDDEN, OUT_DIM), time_blocks=nn.ModuleList([blk() for __ in range(DEPTH)]),
               space_blocks=nn.ModuleList([blk() for __ in range(DEPTH)]))
    m.add_space_attn = True
    return m.to(DEV).eval()


def reference_forward(m, x, sdpa):
    """blocks.py:438-457 and :302-305 in torch operations, with timm's Attention and Mlp."""
    def block(b, x):
        x = x + b.attn.proj(timm_core(b.attn.qkv(b.norm1(x)), sdpa))
        return x + b.mlp.fc2(b.mlp.act(b.mlp.fc1(b.norm2(x))))
    with torch.no_grad():
        x = m.input_transform(x)
        B, N, T, C = x.shape
        j = 0
        for i in range(len(m.time_blocks)):
            x = block(m.time_blocks[i], x.reshape(B * N, T, C)).reshape(B, N, T, C)
            if i % (len(m.time_blocks) // len(m.space_blocks)) == 0:
                x_space = block(m.space_blocks[j], x.permute(0, 2, 1, 3).reshape(B * T, N, C))
                x = x_space.reshape(B, T, N, C).permute(0, 2, 1, 3).reshape(B, N, T, C)
                j += 1
        return m.flow_head(x)


def timed(fn, reps, warmup=3):
    wall, dev, peak = [], [], 0
    for r in range(reps + warmup):
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_update_former.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is measured without one")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    q = lambda v: "{:.0f} [{:.0f} .. {:.0f}]".format(*np.quantile(v, [0.5, 0.1, 0.9]))

    def measure(table, indent="  "):
        ref = table["new"]().clone()
        diffs = {f: float((fn().double() - ref.double()).abs().max()) for f, fn in table.items() if f != "new"}
        t = {f: ([], [], []) for f in table}
        for r in range(2):                                       # alternate the formulations
            for f, fn in table.items():
                w, dv, pk = timed(fn, args.reps // 2)
                t[f][0].append(w)
                t[f][1].append(dv)
                t[f][2].append(pk)
        dev = {f: np.concatenate(v[1]) for f, v in t.items()}
        out(indent + "max |new - other|: " + ", ".join(f"{f} {d:.2e}" for f, d in diffs.items()))
        for f, v in t.items():
            ratio = "" if f == "new" else f" = {np.median(dev[f]) / np.median(dev['new']):.2f}x new"
            out(indent + f"{f:7s} device (events) {q(dev[f])} us{ratio}; host wall {q(np.concatenate(v[0]))} us; peak memory a call adds {max(v[2]) / 1e6:.1f} MB")
        return dev

    out(f"update transformer on {torch.cuda.get_device_name(0)}: bt_attention (new) against the torch formulations (matmul, sdpa)")
    out(f"S = {S}, hidden {HIDDEN}, {HEADS} heads of {HD}; alternating, {args.reps} calls each; us median [10 % .. 90 %]")
    model = make_model()
    for name, N in SHAPES:
        out(f"{name}: N = {N}, {N * S} tokens; a float32 score tensor of the space axis would be {HEADS * S * N * N * 4 / 1e9:.2f} GB")
        for what, table in core_calls(N).items():
            out(f"  attention core, {what}:")
            dev = measure(table, "    ")
            if what == "space axis":
                flop = 4.0 * N * N * HD * HEADS * S
                rate = flop / (np.median(dev["new"]) * 1e-6)
                out(f"    space kernel: {flop / 1e9:.1f} GFLOP a call, {rate / 1e12:.1f} TFLOP/s achieved = {100 * rate / MFMA_F32_PEAK:.0f} % of the "
                    f"{MFMA_F32_PEAK / 1e12:.0f} TF float32 MFMA rate (compute bound: the call moves {N * S * 4 * HIDDEN * 4 / 1e6:.0f} MB)")
        x = torch.randn(1, N, S, IN_DIM, device=DEV, generator=torch.Generator(device=DEV).manual_seed(N))
        out(f"  UpdateFormer.forward, {DEPTH} time + {DEPTH} space blocks:")
        measure(dict(new=lambda: uf.forward(model, x), matmul=lambda: reference_forward(model, x, False), sdpa=lambda: reference_forward(model, x, True)), "    ")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
