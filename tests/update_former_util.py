"""Shared by the update-transformer tests and tests/golden/make_golden_update_former.py: the seeded weights and inputs of the
fixture's cases, a torch restatement of the reference's UpdateFormer (main/frontend/core/cotracker/blocks.py:388-457) on
[N * S, C] rows with the attention written as an explicit gather over the row index b * seq_stride + i * tok_stride (the index
specification of include/batrack_attn.h), and a module tree with the attribute names timm gives (no timm needed)."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "update_former.npz")

HIDDEN, HEADS, HEAD_DIM, INPUT_DIM, OUTPUT_DIM, MLP = 96, 2, 48, 40, 19, 384
EPS = 1e-6
# a: a tile tail on both axes; b: the every-other interleave (4 time blocks, 2 space blocks); c: two key tiles on the space axis
CASES = dict(a=dict(seed=71, time_depth=2, space_depth=2, N=37, S=12),
             b=dict(seed=72, time_depth=4, space_depth=2, N=70, S=5),
             c=dict(seed=73, time_depth=2, space_depth=1, N=130, S=12))


def digest(a):
    """Three float64 sums that move when any element of the array does."""
    a = np.asarray(a, np.float64).ravel()
    return np.array([a.sum(), (a * a).sum(), (a * (np.arange(a.size) % 97)).sum()])


def linear_names(time_depth, space_depth):
    """(state_dict prefix, out features, in features) of every Linear, in the order the weights are drawn."""
    names = [("input_transform", HIDDEN, INPUT_DIM), ("flow_head", OUTPUT_DIM, HIDDEN)]
    for group, depth in (("time_blocks", time_depth), ("space_blocks", space_depth)):
        for i in range(depth):
            p = f"{group}.{i}."
            names += [(p + "attn.qkv", 3 * HIDDEN, HIDDEN), (p + "attn.proj", HIDDEN, HIDDEN),
                      (p + "mlp.fc1", MLP, HIDDEN), (p + "mlp.fc2", HIDDEN, MLP)]
    return names


def make_inputs(seed, time_depth, space_depth, N, S, **_):
    """Weights drawn in float64, scaled by 1 / sqrt(fan_in), non-zero biases, all rounded to float32 (returned as float64);
    keyed as the reference's state_dict, and the input under "x" [1, N, S, INPUT_DIM]."""
    rng = np.random.default_rng(seed)
    d = {}
    for name, fo, fi in linear_names(time_depth, space_depth):
        d[name + ".weight"] = rng.standard_normal((fo, fi)) / np.sqrt(fi)
        d[name + ".bias"] = 0.1 * rng.standard_normal(fo)
    d["x"] = rng.standard_normal((1, N, S, INPUT_DIM))
    return {k: v.astype(np.float32).astype(np.float64) for k, v in d.items()}


def case_tensors(c, dtype=torch.float32, device="cpu"):
    return {k: torch.as_tensor(v, dtype=dtype, device=device) for k, v in make_inputs(**CASES[c]).items()}


# ------------------------------------------------------------------------------------------------------------ attention
def softmax_attention(q, k, v, scale):
    """timm's Attention core on [..., L, head_dim]: (q * scale) @ k^T -> softmax -> @ v."""
    return ((q * scale) @ k.transpose(-2, -1)).softmax(dim=-1) @ v


def attention_gather(qkv, heads, n_seq, L, seq_stride, tok_stride, scale=None, hd=HEAD_DIM):
    """qkv [rows, >= 3 heads hd] -> [rows, heads hd]: token i of sequence b is row b * seq_stride + i * tok_stride; rows that no
    token addresses stay zero."""
    scale = hd ** -0.5 if scale is None else scale
    C = heads * hd
    idx = (torch.arange(n_seq, device=qkv.device)[:, None] * seq_stride + torch.arange(L, device=qkv.device)[None, :] * tok_stride)
    g = qkv[idx.reshape(-1), :3 * C].reshape(n_seq, L, 3, heads, hd).permute(2, 0, 3, 1, 4)              # [3, n_seq, heads, L, hd]
    o = softmax_attention(g[0], g[1], g[2], scale).permute(0, 2, 1, 3).reshape(n_seq * L, C)
    out = qkv.new_zeros(qkv.shape[0], C)
    out[idx.reshape(-1)] = o
    return out


def attention_rearranged(qkv, heads, N, S, axis, scale=None, hd=HEAD_DIM):
    """The reference's formulation on x [N, S, .]: rearrange to (b n) t c or (b t) n c, timm's reshape and permute, and back."""
    scale = hd ** -0.5 if scale is None else scale
    C = heads * hd
    x = qkv[:, :3 * C].reshape(N, S, 3 * C)
    if axis == "space":
        x = x.permute(1, 0, 2)
    B, L = x.shape[:2]
    g = x.reshape(B, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
    o = softmax_attention(g[0], g[1], g[2], scale).transpose(1, 2).reshape(B, L, C)
    if axis == "space":
        o = o.permute(1, 0, 2)
    return o.reshape(N * S, C)


# ---------------------------------------------------------------------------------------------------------- restatement
def block(x, T, prefix, axis, N, S, attention=attention_gather):
    lin = lambda v, name: F.linear(v, T[prefix + name + ".weight"], T[prefix + name + ".bias"])
    ln = lambda v: F.layer_norm(v, (v.shape[-1],), None, None, EPS)
    qkv = lin(ln(x), "attn.qkv")
    a = attention(qkv, HEADS, N, S, S, 1) if axis == "time" else attention(qkv, HEADS, S, N, 1, S)
    x = x + lin(a, "attn.proj")
    return x + lin(F.gelu(lin(ln(x), "mlp.fc1"), approximate="tanh"), "mlp.fc2")


def transformer(T, spec, attention=attention_gather):
    """T: case_tensors(...) in any dtype, on any device -> [1, N, S, OUTPUT_DIM]."""
    N, S, td, sd = spec["N"], spec["S"], spec["time_depth"], spec["space_depth"]
    x = F.linear(T["x"].reshape(N * S, INPUT_DIM), T["input_transform.weight"], T["input_transform.bias"])
    j = 0
    for i in range(td):
        x = block(x, T, f"time_blocks.{i}.", "time", N, S, attention)
        if i % (td // sd) == 0:
            x = block(x, T, f"space_blocks.{j}.", "space", N, S, attention)
            j += 1
    return F.linear(x, T["flow_head.weight"], T["flow_head.bias"]).reshape(1, N, S, OUTPUT_DIM)


# ---------------------------------------------------------------------------------------------------------- module tree
class Tree(nn.Module):
    """A plain module that carries what it is given."""
    def __init__(self, **children):
        super().__init__()
        for k, v in children.items():
            setattr(self, k, v)


def _linear(T, name):
    w, b = T[name + ".weight"], T[name + ".bias"]
    m = nn.Linear(w.shape[1], w.shape[0]).to(device=w.device, dtype=w.dtype)
    m.weight.data.copy_(w)
    m.bias.data.copy_(b)
    return m


def _attn_block(T, p, heads=HEADS):
    attn = Tree(qkv=_linear(T, p + "attn.qkv"), proj=_linear(T, p + "attn.proj"), q_norm=nn.Identity(), k_norm=nn.Identity(),
                attn_drop=nn.Dropout(0.0), proj_drop=nn.Dropout(0.0))
    attn.num_heads, attn.scale = heads, (T[p + "attn.qkv.weight"].shape[0] // 3 // heads) ** -0.5
    mlp = Tree(fc1=_linear(T, p + "mlp.fc1"), act=nn.GELU(approximate="tanh"), drop1=nn.Dropout(0.0), fc2=_linear(T, p + "mlp.fc2"),
               drop2=nn.Dropout(0.0))
    return Tree(norm1=nn.LayerNorm(HIDDEN, elementwise_affine=False, eps=EPS), attn=attn,
                norm2=nn.LayerNorm(HIDDEN, elementwise_affine=False, eps=EPS), mlp=mlp)


def module_tree(T, spec, cls=Tree, heads=HEADS):
    """An `UpdateFormer`-shaped module (class `cls`) with the attribute names of the reference and of timm, from the tensors T."""
    m = cls(input_transform=_linear(T, "input_transform"), flow_head=_linear(T, "flow_head"),
            time_blocks=nn.ModuleList([_attn_block(T, f"time_blocks.{i}.", heads) for i in range(spec["time_depth"])]),
            space_blocks=nn.ModuleList([_attn_block(T, f"space_blocks.{i}.", heads) for i in range(spec["space_depth"])]))
    m.add_space_attn, m.num_heads, m.hidden_size = True, heads, HIDDEN
    return m.eval()
