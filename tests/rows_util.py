"""Shared by the tests of the fused transformer rows (include/batrack_rows.h, batrack_amd/csrc/rows_linear.hip): a CPU
emulation of the kernel's arithmetic in torch, written from the specification and not from update_former.py — the operand split
into f16 pairs, the weight's power-of-two scale, three (f16x3) or one (f16) float32 matmuls of the parts cast back to float,
the LayerNorm prologue and the GELU / residual epilogue — and the transformer of update_former_util with its Linears swapped
for it.  The emulation keeps the three products in separate accumulators and adds them at the end."""
import math

import torch
import torch.nn.functional as F

import update_former_util as U

F16_MAX = 65504.0


def split16(v):
    """v float32 -> (hi, lo) f16: hi = f16(clamp(v)), lo = f16(clamp(v - float(hi))); NaN passes through the clamp."""
    v = v.float()
    clamp = lambda t: torch.where(t > F16_MAX, torch.full_like(t, F16_MAX), torch.where(t < -F16_MAX, torch.full_like(t, -F16_MAX), t))
    hi = clamp(v).half()
    lo = clamp(v - hi.float()).half()
    return hi, lo


def weight_scale(W):
    """s = 2^floor(log2(1 / max |W|)) clamped to [2^-14, 2^14]; 1 for an all-zero matrix."""
    m = float(W.detach().abs().max())
    if m == 0.0:
        return 1.0
    e = math.floor(math.log2(1.0 / m))
    return 2.0 ** min(14, max(-14, e))


def pack(W):
    s = weight_scale(W)
    ws = W.detach().float() * s
    hi = ws.half()
    lo = (ws - hi.float()).half()
    return hi, lo, 1.0 / s


def emu_linear(a, W, b, precision="f16x3"):
    """(a . W^T) / s + b with the operands split: hi.hi + (hi.lo + lo.hi) for "f16x3", hi.hi alone for "f16"."""
    a_hi, a_lo = split16(a)
    w_hi, w_lo, inv = pack(W)
    acc = a_hi.float() @ w_hi.float().t()
    if precision == "f16x3":
        acc = acc + (a_hi.float() @ w_lo.float().t() + a_lo.float() @ w_hi.float().t())
    else:
        assert precision == "f16"
    acc = acc * inv
    return acc if b is None else acc + b.float()


def statement(x, W, b, norm_eps=None, gelu=False, residual=None, linear=F.linear):
    """residual + act(LayerNorm(x) . W^T + b) in the dtype of its arguments: the torch statements that one launch replaces."""
    a = x if norm_eps is None else F.layer_norm(x, (x.shape[-1],), None, None, norm_eps)
    v = linear(a, W, b)
    if gelu:
        v = F.gelu(v, approximate="tanh")
    return v if residual is None else residual + v


def emu_rows_linear(x, W, b, norm_eps=None, gelu=False, residual=None, precision="f16x3"):
    return statement(x.float(), W, b, norm_eps, gelu, residual, linear=lambda a, W, b: emu_linear(a, W, b, precision))


def emu_block(x, T, prefix, axis, N, S, precision):
    lin = lambda v, name, **k: emu_rows_linear(v, T[prefix + name + ".weight"], T[prefix + name + ".bias"], precision=precision, **k)
    qkv = lin(x, "attn.qkv", norm_eps=U.EPS)
    a = U.attention_gather(qkv, U.HEADS, N, S, S, 1) if axis == "time" else U.attention_gather(qkv, U.HEADS, S, N, 1, S)
    x = lin(a, "attn.proj", residual=x)
    return lin(lin(x, "mlp.fc1", norm_eps=U.EPS, gelu=True), "mlp.fc2", residual=x)


def emu_transformer(T, spec, precision="f16x3"):
    """update_former_util.transformer on float32 tensors with every Linear replaced by the emulation."""
    N, S, td, sd = spec["N"], spec["S"], spec["time_depth"], spec["space_depth"]
    x = emu_linear(T["x"].reshape(N * S, U.INPUT_DIM), T["input_transform.weight"], T["input_transform.bias"], precision)
    j = 0
    for i in range(td):
        x = emu_block(x, T, f"time_blocks.{i}.", "time", N, S, precision)
        if i % (td // sd) == 0:
            x = emu_block(x, T, f"space_blocks.{j}.", "space", N, S, precision)
            j += 1
    return emu_linear(x, T["flow_head.weight"], T["flow_head.bias"], precision).reshape(1, N, S, U.OUTPUT_DIM)


# ------------------------------------------------------------------------------------------------- one call against float64
def make_case(rows, K, Nout, seed=0, bias=True, x=None, W=None):
    """Seeded CPU float32 operands of one rows_linear call: x [rows, K], W [Nout, K] / sqrt(K), bias, residual."""
    g = torch.Generator().manual_seed(1000 * K + Nout + seed)
    x = 1.5 * torch.randn(rows, K, generator=g) + 0.3 if x is None else x
    W = torch.randn(Nout, K, generator=g) / math.sqrt(K) if W is None else W
    b = 0.1 * torch.randn(Nout, generator=g) if bias else None
    return dict(x=x, W=W, b=b, res=torch.randn(rows, Nout, generator=g))


def linear_module(W, b, device):
    lin = torch.nn.Linear(W.shape[1], W.shape[0], bias=b is not None).to(device)
    lin.weight.data.copy_(W)
    if b is not None:
        lin.bias.data.copy_(b)
    return lin.eval()


def gates(c, norm_eps, gelu, residual, precision):
    """(float64 truth, gate): twice the error of torch's float32 run of the statement on the CPU ("f16x3"), or twice the
    error of the hi-only emulation ("f16"), both against the same statement in float64."""
    d = lambda t: None if t is None else t.double()
    res = c["res"] if residual else None
    truth = statement(d(c["x"]), d(c["W"]), d(c["b"]), norm_eps, gelu, d(res))
    if precision == "f16x3":
        mine = statement(c["x"], c["W"], c["b"], norm_eps, gelu, res)
    else:
        mine = emu_rows_linear(c["x"], c["W"], c["b"], norm_eps, gelu, res, "f16")
    return truth, 2 * float((mine.double() - truth).abs().max()) if truth.numel() else 0.0
