"""The attention kernels at their limits (batrack_amd/csrc/attention.hip, include/batrack_attn.h): sequence lengths around the
wave's 32 queries, the workgroup's 128 and the key tile's 64, one head and one sequence, scales other than the default, logits
large enough that the softmax is one-hot and the running maximum moves between key tiles, logits of 1e37, the reach of a
non-finite k, and misaligned pointers through the raw entry.

Tolerances.  No bound is derived from the kernel under test.  The convention of tests/test_gpu_attention.py, unchanged:
    max |kernel - float64| <= 2 x max |torch's float32 formulation - float64|   on the same inputs on the same GPU.
Where a second bound is asserted it is a-priori: a softmax-weighted mean of L values of v, summed in float32 in any order
and divided once, is within 4 u L max |v| of the exact one (u = 2^-24), whatever the weights."""
import math

import pytest
import torch

import test_gpu_attention as A
import update_former_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HD = A.HD
UNIT = 2.0 ** -24
uf, layout, raw = A.uf, A.layout, A.raw


def compare_scaled(qkv, heads, n_seq, L, ss, ts, scale, what):
    """A.compare with a scale: -> (kernel, float64 truth, torch's float32 run)."""
    got = uf().attention(qkv, heads, n_seq, L, ss, ts, scale)
    truth = U.attention_gather(qkv.double(), heads, n_seq, L, ss, ts, scale)
    ref32 = U.attention_gather(qkv, heads, n_seq, L, ss, ts, scale)
    e_ker, e_ref = float((got.double() - truth).abs().max()), float((ref32.double() - truth).abs().max())
    print(f"{what}: max |kernel - f64| {e_ker:.3e}, max |torch float32 - f64| {e_ref:.3e}")
    assert got.shape == (qkv.shape[0], heads * HD) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all()), what
    if bool(torch.isfinite(ref32).all()):
        assert e_ker <= 2 * e_ref, (what, e_ker, e_ref)
    else:                                                               # torch's own float32 run overflowed: the a-priori bound
        vmax = float(qkv[:, 2 * heads * HD:3 * heads * HD].abs().max())
        assert e_ker <= 4 * UNIT * L * vmax, (what, e_ker, vmax)
    return got, truth, ref32


def random_qkv(n_seq, L, heads, seed, factor=1.0):
    qkv = torch.randn(n_seq * L, 3 * heads * HD, generator=torch.Generator().manual_seed(seed))
    qkv[:, :2 * heads * HD] *= factor
    return qkv.to(DEV)


@pytest.mark.parametrize("n_seq,heads", [(1, 1), (5, 3), (2, 8)])
@pytest.mark.parametrize("kind", ["time", "space"])
@pytest.mark.parametrize("L", [31, 32, 33, 127, 128, 129, 191, 192, 193, 256])
def test_tails_at_the_query_and_wave_tiles(L, kind, n_seq, heads):
    """Every L at which a query tile of 16, a wave's 32 queries, the workgroup's 128 or a key tile of 64 ends, one short and one over."""
    ss, ts = layout(kind, n_seq, L)
    A.compare(random_qkv(n_seq, L, heads, 6000 + 10 * L + heads), heads, n_seq, L, ss, ts, f"L={L} {kind} n_seq={n_seq} heads={heads}")


@pytest.mark.parametrize("kind", ["time", "space"])
@pytest.mark.parametrize("L", [12, 130])
@pytest.mark.parametrize("scale", [0.0, -0.3, 1.0, 1e-30])
def test_scales(scale, L, kind):
    """At scale 0 every logit is 0 and the result is the mean of v: additionally within 4 u L max |v| of the float64 mean."""
    n_seq, heads = 5, 3
    ss, ts = layout(kind, n_seq, L)
    qkv = random_qkv(n_seq, L, heads, 7000 + L)
    got, _, _ = compare_scaled(qkv, heads, n_seq, L, ss, ts, scale, f"scale={scale:g} L={L} {kind}")
    if scale == 0.0:
        C = heads * HD
        idx = torch.arange(n_seq, device=DEV)[:, None] * ss + torch.arange(L, device=DEV)[None, :] * ts
        v = qkv[idx.reshape(-1), 2 * C:].double().reshape(n_seq, L, C)
        mean = v.mean(1, keepdim=True).expand(n_seq, L, C).reshape(n_seq * L, C)
        err = float((got[idx.reshape(-1)].double() - mean).abs().max())
        print(f"scale=0 L={L} {kind}: max |kernel - mean of v| {err:.3e}, bound {4 * UNIT * L * float(v.abs().max()):.3e}")
        assert err <= 4 * UNIT * L * float(v.abs().max())


@pytest.mark.parametrize("kind,L", [("time", 12), ("space", 12), ("time", 193), ("space", 193)])
@pytest.mark.parametrize("factor", [8.0, 25.0])
def test_large_logits(factor, kind, L):
    """q and k scaled by 8 and by 25: logits of standard deviation 64 and 625, a softmax near one-hot whose maximum sits
    in any key tile."""
    n_seq, heads = 3, 2
    ss, ts = layout(kind, n_seq, L)
    compare_scaled(random_qkv(n_seq, L, heads, 8000 + L, factor), heads, n_seq, L, ss, ts, HD ** -0.5, f"q, k x {factor:g} L={L} {kind}")


def rows_of(qkv5, kind):
    """[n_seq, L, 3, heads, HD] -> the kernel's rows for the layout."""
    n_seq, L = qkv5.shape[:2]
    if kind == "space":
        qkv5 = qkv5.permute(1, 0, 2, 3, 4)
    return qkv5.reshape(n_seq * L, -1).contiguous().float().to(DEV)


@pytest.mark.parametrize("kind", ["time", "space"])
def test_row_maximum_in_the_first_and_in_the_last_key_tile(kind):
    """L = 193: four key tiles, the last of one key.  q_i = 3 k_target(i) with k of standard deviation 3: the logit of
    the target is about 190, the others are of standard deviation 27.  Even queries aim at a key of the first tile (the
    running maximum is set at once and every later tile is rescaled against it), odd queries at key 192 (the maximum arrives
    with the last tile and rescales all that was accumulated)."""
    n_seq, heads, L = 2, 2, 193
    ss, ts = layout(kind, n_seq, L)
    g = torch.Generator().manual_seed(8500)
    qkv = torch.randn(n_seq, L, 3, heads, HD, generator=g)
    qkv[:, :, 1] *= 3
    target = torch.where(torch.arange(L) % 2 == 0, torch.arange(L) % 64, torch.full((L,), L - 1))
    qkv[:, :, 0] = 3 * qkv[:, target, 1]
    got, truth, _ = compare_scaled(rows_of(qkv, kind), heads, n_seq, L, ss, ts, HD ** -0.5, f"maximum first / last tile {kind}")
    logits = torch.einsum("bihd,bjhd->bhij", qkv[:, :, 0].double(), qkv[:, :, 1].double())
    assert torch.equal(logits.argmax(-1), target[None, None].expand(n_seq, heads, L))       # the construction does what it says


@pytest.mark.parametrize("kind,L", [("time", 12), ("space", 193)])
def test_logits_of_1e37(kind, L):
    """q and k of size 1e18 in all 48 columns: 24 copies of a point on a circle, so that q_i . k_j = 2.4e37 cos(angle):
    finite in every partial sum, and the best key leads the second by 2.4e37 (1 - cos(2 pi / L)), far above the rounding of a
    48-term float32 sum of such products.  The softmax is one-hot; the output must be finite and under the convention."""
    n_seq, heads = 2, 2
    ss, ts = layout(kind, n_seq, L)
    g = torch.Generator().manual_seed(8600 + L)
    theta = 2 * math.pi * torch.arange(L, dtype=torch.float64) / L
    qkv = torch.zeros(n_seq, L, 3, heads, HD, dtype=torch.float64)
    qkv[:, :, 1, :, 0::2], qkv[:, :, 1, :, 1::2] = 1e18 * theta.cos()[None, :, None, None], 1e18 * theta.sin()[None, :, None, None]
    perm = torch.stack([torch.stack([torch.randperm(L, generator=g) for __ in range(heads)]) for __ in range(n_seq)])
    for b in range(n_seq):
        for h in range(heads):
            qkv[b, :, 0, h] = qkv[b, perm[b, h], 1, h]
    qkv[:, :, 2] = torch.randn(n_seq, L, heads, HD, generator=g, dtype=torch.float64)
    rows = rows_of(qkv, kind)
    C = heads * HD
    assert bool(torch.isfinite(rows).all()) and 2e37 < float((rows[:, :C].double() @ rows[:, C:2 * C].double().t()).abs().max()) < 1e38
    compare_scaled(rows, heads, n_seq, L, ss, ts, HD ** -0.5, f"logits of 1e37 L={L} {kind}")


@pytest.mark.parametrize("kind,L", [("time", 12), ("space", 130)])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_reach_of_a_non_finite_k(bad, kind, L):
    """A NaN, then +inf, in one token's k: every output outside that sequence and head has the clean run's bits; inside
    it the output differs from the clean run."""
    n_seq, heads = 5, 3
    ss, ts = layout(kind, n_seq, L)
    C = heads * HD
    qkv = random_qkv(n_seq, L, heads, 9000 + L)
    clean = uf().attention(qkv, heads, n_seq, L, ss, ts)
    b, i, h = 3, L - 2, 1
    dirty = qkv.clone()
    dirty[b * ss + i * ts, C + h * HD + 7] = bad
    out = uf().attention(dirty, heads, n_seq, L, ss, ts)
    cell = torch.zeros_like(out, dtype=torch.bool)
    cell[b * ss + torch.arange(L, device=DEV) * ts, h * HD:(h + 1) * HD] = True
    assert torch.equal(out[~cell], clean[~cell])
    assert not torch.equal(out[cell], clean[cell])


@pytest.mark.parametrize("kind,L", [("time", 12), ("space", 130)])
def test_pointers_off_the_16_byte_grid(kind, L):
    """qkv moved by 4 bytes with row strides that stay multiples of 4 floats, then out alone moved: the scalar path, the
    same arithmetic in the same order as the float4 path — bit-equal to the aligned call."""
    n_seq, heads = 5, 3
    ss, ts = layout(kind, n_seq, L)
    C, rows = heads * HD, n_seq * L
    qs, os_ = 3 * C + 4, C + 8
    qkv = random_qkv(n_seq, L, heads, 9500 + L)
    sentinel = -12345.5

    def call(q_off, o_off):
        """q_off, o_off: floats by which the two buffers are moved off their 16-byte aligned allocation."""
        qbuf = torch.full((rows * qs + 8,), float("nan"), device=DEV)
        qbuf[q_off:q_off + rows * qs].view(rows, qs)[:, :3 * C] = qkv
        obuf = torch.full((rows * os_ + 8,), sentinel, device=DEV)
        assert qbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
        raw(qbuf.data_ptr() + 4 * q_off, qs, obuf.data_ptr() + 4 * o_off, os_, n_seq, L, ss, ts, heads, HD ** -0.5)
        torch.cuda.synchronize()
        out = obuf[o_off:o_off + rows * os_].view(rows, os_)
        assert bool((out[:, C:] == sentinel).all()) and bool((obuf[:o_off] == sentinel).all()) and bool((obuf[o_off + rows * os_:] == sentinel).all())
        return out[:, :C].clone()

    aligned = call(0, 0)
    assert torch.equal(aligned, uf().attention(qkv, heads, n_seq, L, ss, ts))
    assert torch.equal(call(1, 0), aligned)
    assert torch.equal(call(0, 1), aligned)
    assert torch.equal(call(3, 2), aligned)
