"""The tracker's update transformers (the reference's main/frontend/core/cotracker/blocks.py:388-457, `UpdateFormer`, and
:280-305, `AttnBlock`) with the attention core in HIP (batrack_amd/csrc/attention.hip through include/batrack_attn.h, which
holds the specification).  x stays [N * S, C] rows (token (n, t) is row n * S + t) for the whole transformer: the row-wise
parts of a block are torch operations on those rows, and only the attention knows the axis, through two strides.

    attention(qkv [rows, >= 3 heads 48], heads, n_seq, L, seq_stride, tok_stride, scale=None) -> [rows, heads 48]   one launch
    attn_block(x [N S, C], blk, axis, N, S) -> [N S, C]       one AttnBlock; axis "time" or "space"
    forward(self, input_tensor [1, N, T, input_dim]) -> [1, N, T, output_dim]      the reference's signature and return

Inference only (inputs are detached, no autograd through the kernel), GPU tensors only; no CPU fallback.  B = 1, heads of 48.
What it cannot do raises a RuntimeError that names the reason; there is no route to another path.

`install()` makes the reference's `UpdateFormer` use `forward`; with track_iter.install() the two compose."""
import importlib

import torch
import torch.nn.functional as F

from .. import _lib

HEAD_DIM = 48                # BT_ATTN_HEAD_DIM


def _gpu(name, t, what="update_former"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: `{name}` must be a tensor on the GPU (there is no CPU fallback in batrack_amd)")
    return t.detach().float()


def attention(qkv, heads, n_seq, L, seq_stride, tok_stride, scale=None):
    """Token i of sequence b is row b * seq_stride + i * tok_stride of `qkv` and of the result; within a row q, k and v of
    head h are at columns h * 48, (heads + h) * 48 and (2 heads + h) * 48.  Rows that no token addresses are left unwritten."""
    qkv = _gpu("qkv", qkv, "attention")
    heads, n_seq, L, seq_stride, tok_stride = int(heads), int(n_seq), int(L), int(seq_stride), int(tok_stride)
    C = heads * HEAD_DIM
    if qkv.dim() != 2 or heads < 1 or qkv.shape[1] < 3 * C:
        raise RuntimeError(f"attention: qkv must be [rows, >= 3 * heads * {HEAD_DIM}], got {tuple(qkv.shape)} for {heads} heads")
    if qkv.shape[1] > 1 and qkv.stride(1) != 1 or (qkv.shape[0] > 1 and qkv.stride(0) < 3 * C):
        qkv = qkv.contiguous()
    scale = HEAD_DIM ** -0.5 if scale is None else float(scale)
    ops = _lib.torch_ops()
    if ops is not None:
        return ops.attention(qkv, heads, n_seq, L, seq_stride, tok_stride, scale)
    rows = qkv.shape[0]
    if n_seq < 0 or L < 1 or seq_stride < 1 or tok_stride < 1 or (n_seq and (n_seq - 1) * seq_stride + (L - 1) * tok_stride >= rows):
        raise RuntimeError("attention: a token addresses a row past the end of qkv")
    out = torch.empty(rows, C, dtype=torch.float32, device=qkv.device)
    if n_seq and rows:
        _lib.check(_lib.lib().bt_attention(qkv.data_ptr(), qkv.stride(0) if rows > 1 else qkv.shape[1], out.data_ptr(), C, n_seq, L,
                                           seq_stride, tok_stride, heads, HEAD_DIM, scale,
                                           torch.cuda.current_stream(qkv.device).cuda_stream), "bt_attention")
    return out


def _check_block(blk, C, training):
    heads = int(blk.attn.num_heads)
    if heads < 1 or C % heads or C // heads != HEAD_DIM:
        raise RuntimeError(f"update_former: heads of {C}/{heads} columns; the attention kernel is built for heads of {HEAD_DIM}")
    for name in ("q_norm", "k_norm"):
        norm = getattr(blk.attn, name, None)
        if norm is not None and not isinstance(norm, torch.nn.Identity):
            raise RuntimeError(f"update_former: attn.{name} is not an identity; the attention kernel normalises neither q nor k")
    if training:
        for owner, name in ((blk.attn, "attn_drop"), (blk.attn, "proj_drop"), (blk.mlp, "drop1"), (blk.mlp, "drop2"), (blk.mlp, "drop")):
            if float(getattr(getattr(owner, name, None), "p", 0.0)) != 0.0:
                raise RuntimeError(f"update_former: {name} has non-zero dropout in training mode; this forward is inference only")
    return heads


def _layer_norm(x, norm):
    w, b = getattr(norm, "weight", None), getattr(norm, "bias", None)
    return F.layer_norm(x, (x.shape[-1],), None if w is None else w.detach(), None if b is None else b.detach(), norm.eps)


def _linear(x, lin):
    return F.linear(x, lin.weight.detach(), None if lin.bias is None else lin.bias.detach())


def attn_block(x, blk, axis, N, S):
    """One AttnBlock on x [N * S, C]; `axis` is "time" (N sequences of S tokens) or "space" (S sequences of N tokens)."""
    x = _gpu("x", x, "attn_block")
    if axis not in ("time", "space"):
        raise RuntimeError(f"attn_block: axis must be 'time' or 'space', got {axis!r}")
    if x.dim() != 2 or x.shape[0] != N * S:
        raise RuntimeError(f"attn_block: x must be [N * S, C] = [{N * S}, C], got {tuple(x.shape)}")
    heads = _check_block(blk, x.shape[1], False)
    with torch.no_grad():
        qkv = _linear(_layer_norm(x, blk.norm1), blk.attn.qkv)
        scale = float(getattr(blk.attn, "scale", HEAD_DIM ** -0.5))
        a = attention(qkv, heads, N, S, S, 1, scale) if axis == "time" else attention(qkv, heads, S, N, 1, S, scale)
        x = x + _linear(a, blk.attn.proj)
        return x + _linear(blk.mlp.act(_linear(_layer_norm(x, blk.norm2), blk.mlp.fc1)), blk.mlp.fc2)


def forward(self, input_tensor):
    x = _gpu("input_tensor", input_tensor, "UpdateFormer.forward")
    if x.dim() != 4 or x.shape[0] != 1:
        raise RuntimeError(f"UpdateFormer.forward: input [B, N, T, C] with B = 1 (B > 1 is not built), got {tuple(x.shape)}")
    B, N, T, __ = x.shape
    time_blocks = list(self.time_blocks)
    space_blocks = list(self.space_blocks) if getattr(self, "add_space_attn", True) else []
    C = self.input_transform.weight.shape[0]
    training = bool(getattr(self, "training", False))
    for blk in time_blocks + space_blocks:
        _check_block(blk, C, training)
    with torch.no_grad():
        x = _linear(x.reshape(N * T, -1), self.input_transform)
        j = 0
        for i, blk in enumerate(time_blocks):
            x = attn_block(x, blk, "time", N, T)
            if space_blocks and i % (len(time_blocks) // len(space_blocks)) == 0:
                x = attn_block(x, space_blocks[j], "space", N, T)
                j += 1
        return _linear(x, self.flow_head).reshape(B, N, T, -1)


def install(module=None):
    """Set `UpdateFormer.forward` in the reference's `main.frontend.core.cotracker.blocks` (or in the module given) to the
    function above; returns what was bound before.  Opt-in: nothing in batrack_amd calls it."""
    if module is None:
        module = importlib.import_module("main.frontend.core.cotracker.blocks")
    previous = getattr(module.UpdateFormer, "forward", None)
    module.UpdateFormer.forward = forward
    return previous
