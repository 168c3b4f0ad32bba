"""GPU half of the attention core (batrack_amd/csrc/attention.hip, include/batrack_attn.h): exact selection (any transposition,
permuted-k mismatch or mis-strided row shows as a wrong row), the tails of both paths against float64 on the same GPU under
twice the error of torch's own float32 formulation on the same inputs, padded rows, the reach of a NaN, repetition, and one
real-shape case per axis.  No bound is derived from the kernel under test.

Why twice: a float32 kernel that sums in another order carries rounding of the same size as the float32 reference's own
(0.7-1.4 x in a CPU emulation of L = 12, 130, 700); a bf16 operand or a fast-math exponential misses it by orders of magnitude."""
import math

import pytest
import torch

import update_former_util as U
from batrack_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HD = 48


def uf():
    from batrack_amd.frontend import update_former
    return update_former


def layout(kind, n_seq, L):
    """(seq_stride, tok_stride) of the two axes of a [., .] token grid."""
    return (L, 1) if kind == "time" else (1, n_seq)


def raw(qkv_ptr, qs, out_ptr, os_, n_seq, L, ss, ts, heads, scale):
    rc = _lib.lib().bt_attention(qkv_ptr, qs, out_ptr, os_, n_seq, L, ss, ts, heads, HD, scale, torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.BT_OK, rc


def reference(qkv, heads, n_seq, L, ss, ts, dtype):
    """The gather formulation of tests/update_former_util.py in `dtype`, one sequence at a time when the scores are large."""
    q = qkv.to(dtype)
    if L <= 256:
        return U.attention_gather(q, heads, n_seq, L, ss, ts)
    out = q.new_zeros(q.shape[0], heads * HD)
    for b in range(n_seq):
        idx = b * ss + torch.arange(L, device=q.device) * ts
        out[idx] = U.attention_gather(q[idx], heads, 1, L, L, 1)
    return out


def compare(qkv, heads, n_seq, L, ss, ts, what):
    got = uf().attention(qkv, heads, n_seq, L, ss, ts)
    truth = reference(qkv, heads, n_seq, L, ss, ts, torch.float64)
    e_ref = float((reference(qkv, heads, n_seq, L, ss, ts, torch.float32).double() - truth).abs().max())
    e_ker = float((got.double() - truth).abs().max())
    print(f"{what}: max |kernel - f64| {e_ker:.3e}, max |torch float32 - f64| {e_ref:.3e}")
    assert got.shape == (qkv.shape[0], heads * HD) and got.dtype == torch.float32 and got.is_contiguous()
    assert bool(torch.isfinite(got).all())
    assert e_ker <= 2 * e_ref, (what, e_ker, e_ref)
    return got


@pytest.mark.parametrize("kind", ["time", "space"])
@pytest.mark.parametrize("L", [12, 17, 130, 257])
def test_exact_selection(L, kind):
    n_seq, heads = 3, 2
    ss, ts = layout(kind, n_seq, L)
    C = heads * HD
    scale = HD ** -0.5
    g = torch.Generator().manual_seed(1000 + L)
    theta = 2 * math.pi * torch.arange(L, dtype=torch.float64) / L
    c = 200.0 / (scale * (1 - math.cos(2 * math.pi / L)))
    qkv = torch.zeros(n_seq, L, 3, heads, HD, dtype=torch.float64)
    qkv[:, :, 1, :, 5], qkv[:, :, 1, :, 31] = theta.cos()[None, :, None], theta.sin()[None, :, None]
    perm = torch.stack([torch.stack([torch.randperm(L, generator=g) for __ in range(heads)]) for __ in range(n_seq)])   # [n_seq, heads, L]
    for b in range(n_seq):
        for h in range(heads):
            qkv[b, :, 0, h] = c * qkv[b, perm[b, h], 1, h]
    qkv[:, :, 2] = torch.randn(n_seq, L, heads, HD, generator=g, dtype=torch.float64)
    qkv = qkv.float()
    rows = qkv.reshape(n_seq * L, 3 * C)                                      # token (b, i) at row b * L + i
    if kind == "space":
        rows = qkv.permute(1, 0, 2, 3, 4).reshape(L * n_seq, 3 * C)         # token (b, i) at row i * n_seq + b
    out = uf().attention(rows.contiguous().to(DEV), heads, n_seq, L, ss, ts, scale).cpu()
    out = out.reshape(n_seq, L, heads, HD) if kind == "time" else out.reshape(L, n_seq, heads, HD).permute(1, 0, 2, 3)
    for b in range(n_seq):
        for h in range(heads):
            assert torch.equal(out[b, :, h], qkv[b, perm[b, h], 2, h]), (b, h)


@pytest.mark.parametrize("kind", ["time", "space"])
@pytest.mark.parametrize("L", [1, 2, 12, 15, 16, 17, 63, 64, 65, 130])
def test_tails(L, kind):
    n_seq, heads = 5, 3
    ss, ts = layout(kind, n_seq, L)
    g = torch.Generator().manual_seed(2000 + L)
    qkv = torch.randn(n_seq * L, 3 * heads * HD, generator=g).to(DEV)
    compare(qkv, heads, n_seq, L, ss, ts, f"tails L={L} {kind}")


@pytest.mark.parametrize("kind,L", [("time", 12), ("space", 12), ("time", 70), ("space", 130)])
def test_padding(kind, L):
    """Row strides with gap columns, NaN in the gaps and in the rows before and after the addressed ones; a sentinel in out."""
    n_seq, heads, pad = 5, 3, 3
    ss, ts = layout(kind, n_seq, L)
    C = heads * HD
    qs, os_ = 3 * C + 7, C + 5
    rows = n_seq * L
    g = torch.Generator().manual_seed(3000 + L)
    clean = torch.randn(rows, 3 * C, generator=g).to(DEV)
    want = uf().attention(clean, heads, n_seq, L, ss, ts)
    buf = torch.full((rows + 2 * pad, qs), float("nan"), device=DEV)
    buf[pad:pad + rows, :3 * C] = clean
    sentinel = -12345.5
    out = torch.full((rows + 2 * pad, os_), sentinel, device=DEV)
    raw(buf.data_ptr() + pad * qs * 4, qs, out.data_ptr() + pad * os_ * 4, os_, n_seq, L, ss, ts, heads, HD ** -0.5)
    torch.cuda.synchronize()
    got = out[pad:pad + rows, :C]
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    assert bool((out[:pad] == sentinel).all()) and bool((out[pad + rows:] == sentinel).all()) and bool((out[:, C:] == sentinel).all())


@pytest.mark.parametrize("kind,L", [("time", 12), ("space", 130)])
def test_isolation(kind, L):
    n_seq, heads = 5, 3
    ss, ts = layout(kind, n_seq, L)
    C = heads * HD
    g = torch.Generator().manual_seed(4000 + L)
    qkv = torch.randn(n_seq * L, 3 * C, generator=g).to(DEV)
    clean = uf().attention(qkv, heads, n_seq, L, ss, ts)
    b, i, h = 3, L - 2, 1
    r = b * ss + i * ts
    # a NaN in one token's q: that token's row of that head, and nothing else
    bad = qkv.clone()
    bad[r, h * HD + 7] = float("nan")
    out = uf().attention(bad, heads, n_seq, L, ss, ts)
    cell = torch.zeros_like(out, dtype=torch.bool)
    cell[r, h * HD:(h + 1) * HD] = True
    assert not bool(torch.isfinite(out[cell]).any())
    assert torch.equal(out[~cell], clean[~cell])
    # a NaN in one token's v: its sequence and head, and nothing else
    bad = qkv.clone()
    bad[r, 2 * C + h * HD + 7] = float("nan")
    out = uf().attention(bad, heads, n_seq, L, ss, ts)
    cell = torch.zeros_like(out, dtype=torch.bool)
    cell[b * ss + torch.arange(L, device=DEV) * ts, h * HD:(h + 1) * HD] = True
    assert torch.equal(out[~cell], clean[~cell])
    assert not torch.equal(out[cell], clean[cell])


def test_repeat_and_empty():
    for n_seq, L, ss, ts in ((7, 12, 12, 1), (3, 200, 1, 3)):
        qkv = torch.randn(n_seq * L, 3 * 2 * HD, generator=torch.Generator().manual_seed(L)).to(DEV)
        assert torch.equal(uf().attention(qkv, 2, n_seq, L, ss, ts), uf().attention(qkv, 2, n_seq, L, ss, ts))
    out = uf().attention(torch.zeros(0, 3 * 2 * HD, device=DEV), 2, 0, 12, 12, 1)
    assert out.shape == (0, 2 * HD) and out.dtype == torch.float32
    with pytest.raises(RuntimeError, match="past the end"):
        uf().attention(torch.zeros(23, 3 * 2 * HD, device=DEV), 2, 2, 12, 12, 1)


@pytest.mark.parametrize("kind", ["time", "space"])
def test_real_shape(kind):
    """S = 12, N = 1536, 8 heads.  The float64 truth of the space axis is formed a frame at a time (150 MB of scores)."""
    S, N, heads = 12, 1536, 8
    n_seq, L = (N, S) if kind == "time" else (S, N)
    ss, ts = layout(kind, n_seq, L)
    qkv = torch.randn(N * S, 3 * heads * HD, generator=torch.Generator().manual_seed(5)).to(DEV)
    compare(qkv, heads, n_seq, L, ss, ts, f"real shape {kind}")
