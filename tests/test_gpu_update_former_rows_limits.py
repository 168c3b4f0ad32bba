"""bt_rows_linear (include/batrack_rows.h) at its limits, through update_former.rows_linear: row, column and K tails, strides
and alignment, aliasing, the activation range, the isolation of non-finite values, zero weights.  The gate is that of
tests/test_gpu_update_former_rows.py: twice the error of torch's float32 run of the same statement on the CPU, against float64.

That gate is the largest error over the outputs of ONE call, so a call with few outputs gives a noisy one: the row cases
therefore take the fixture's widest Linear (K 96 -> 384: a one-row call still has 384 outputs) and the column cases its row count
(37 * 12 = 444: one column still has 444 outputs).  torch's CPU routine for a single row or column is also a different, more
accurate one (a dot product over vector lanes; its error is about half that of the many-row routine), which the gate follows."""
import math

import pytest
import torch

import rows_util as R
import update_former_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -777.0


def uf():
    from batrack_amd.frontend import update_former
    return update_former


def check(c, norm_eps=U.EPS, gelu=True, residual=True, precision="f16x3", what=""):
    """The call on the case `c` against float64 at the gate; returns the result."""
    truth, gate = R.gates(c, norm_eps, gelu, residual, precision)
    lin = R.linear_module(c["W"], c["b"], DEV)
    got = uf().rows_linear(c["x"].to(DEV), lin, norm_eps=norm_eps, gelu=gelu, residual=c["res"].to(DEV) if residual else None, precision=precision)
    assert got.shape == truth.shape
    if truth.numel():
        err = float((got.cpu().double() - truth).abs().max())
        print(f"{what}: max |rows_linear - f64| {err:.3e}, gate {gate:.3e}")
        assert err <= gate, (what, err, gate)
    return got


@pytest.mark.parametrize("rows", [0, 1, 127, 128, 129])
def test_row_counts(rows):
    c = R.make_case(rows, 96, 384)
    for norm_eps, gelu, residual in ((U.EPS, True, True), (None, False, False)):
        got = check(c, norm_eps, gelu, residual, what=f"rows {rows}")
        assert got.shape == (rows, 384) and got.dtype == torch.float32
    if rows == 0:                                                   # nothing is launched: a given `out` comes back as it is
        out = torch.empty(0, 384, device=DEV)
        assert uf().rows_linear(c["x"].to(DEV), R.linear_module(c["W"], c["b"], DEV), out=out) is out


@pytest.mark.parametrize("Nout", [1, 15, 16, 17, 131])
def test_column_counts(Nout):
    c = R.make_case(37 * 12, 96, Nout)
    check(c, what=f"Nout {Nout}")
    check(c, None, False, False, what=f"Nout {Nout}, the Linear alone")
    check(c, None, False, True, precision="f16", what=f"Nout {Nout}, f16")


@pytest.mark.parametrize("K", [8, 24, 32, 40, 456])
def test_k_counts(K):
    c = R.make_case(130, K, 96)
    check(c, what=f"K {K}")
    check(c, None, False, False, what=f"K {K}, the Linear alone")
    check(c, None, True, True, precision="f16", what=f"K {K}, f16")


def test_k_off_the_fragment_is_refused():
    c = R.make_case(16, 12, 24)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        uf().rows_linear(c["x"].to(DEV), R.linear_module(c["W"], c["b"], DEV))
    from batrack_amd import _lib
    ops = _lib.torch_ops(strict=True)
    h = torch.zeros(24, 12, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.rows_linear(c["x"].to(DEV), h, h, 1.0, None, -1.0, False, None, torch.empty(16, 24, device=DEV), 0)


def test_strides_of_x_out_and_residual():
    rows, K, Nout = 130, 40, 19
    c = R.make_case(rows, K, Nout)
    lin = R.linear_module(c["W"], c["b"], DEV)
    x, res = c["x"].to(DEV), c["res"].to(DEV)
    want = check(c, what="contiguous")
    for off, width in ((4, 52), (3, 47)):                           # a column slice on and off the 16-byte grid
        wide = torch.full((rows, width), SENTINEL, device=DEV)
        wide[:, off:off + K] = x
        rbuf = torch.full((rows, Nout + 6), SENTINEL, device=DEV)
        rbuf[:, 5:5 + Nout] = res
        obuf = torch.full((rows, Nout + 9), SENTINEL, device=DEV)
        got = uf().rows_linear(wide[:, off:off + K], lin, norm_eps=U.EPS, gelu=True, residual=rbuf[:, 5:5 + Nout], out=obuf[:, 2:2 + Nout])
        assert got.data_ptr() == obuf[:, 2:].data_ptr() and torch.equal(got, want)
        assert bool((obuf[:, :2] == SENTINEL).all()) and bool((obuf[:, 2 + Nout:] == SENTINEL).all())      # nothing beside the columns
        assert bool((wide[:, :off] == SENTINEL).all()) and bool((rbuf[:, :5] == SENTINEL).all())


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_pointers_off_the_16_byte_grid_are_bit_equal(precision):
    from batrack_amd import _lib
    ops = _lib.torch_ops(strict=True)
    rows, K, Nout = 130, 96, 35
    c = R.make_case(rows, K, Nout)
    lin = R.linear_module(c["W"], c["b"], DEV)
    x = c["x"].to(DEV)
    want = uf().rows_linear(x, lin, norm_eps=U.EPS, gelu=True, precision=precision)
    flat = torch.empty(rows * K + 8, device=DEV)
    xo = flat[1:1 + rows * K].view(rows, K)                         # 4 bytes off
    xo.copy_(x)
    assert x.data_ptr() % 16 == 0 and xo.data_ptr() % 16 == 4
    assert torch.equal(uf().rows_linear(xo, lin, norm_eps=U.EPS, gelu=True, precision=precision), want)
    # the weights 4 bytes off, through the operator itself
    w_hi, w_lo, inv = uf().pack_linear(lin.weight)
    shifted = []
    for w in (w_hi, w_lo):
        buf = torch.empty(Nout * K + 16, dtype=torch.float16, device=DEV)
        s = buf[2:2 + Nout * K].view(Nout, K)
        s.copy_(w)
        assert s.data_ptr() % 16 == 4 and s.is_contiguous()
        shifted.append(s)
    prec = _lib.BT_ROWS_PRECISION[precision]
    for xx in (x, xo):
        out = torch.empty(rows, Nout, device=DEV)
        ops.rows_linear(xx, shifted[0], shifted[1], inv, lin.bias.detach(), U.EPS, True, None, out, prec)
        assert torch.equal(out, want)


def test_out_may_be_the_residual_and_must_not_overlap_x():
    rows, K = 130, 96
    c = R.make_case(rows, K, K)
    lin = R.linear_module(c["W"], c["b"], DEV)
    x, res = c["x"].to(DEV), c["res"].to(DEV)
    want = uf().rows_linear(x, lin, norm_eps=U.EPS, gelu=True, residual=res)
    buf = res.clone()
    got = uf().rows_linear(x, lin, norm_eps=U.EPS, gelu=True, residual=buf, out=buf)
    assert got is buf and torch.equal(buf, want)
    keep = x.clone()
    with pytest.raises(RuntimeError, match="overlaps"):
        uf().rows_linear(x, lin, out=x)
    flat = torch.zeros(rows * K + 4, device=DEV)
    with pytest.raises(RuntimeError, match="overlaps"):
        uf().rows_linear(flat[:rows * K].view(rows, K), lin, out=flat[4:].view(rows, K))
    from batrack_amd import _lib
    w_hi, w_lo, inv = uf().pack_linear(lin.weight)
    with pytest.raises(RuntimeError, match="overlap"):              # the operator's own refusal (the C ABI's BT_EINVAL)
        _lib.torch_ops(strict=True).rows_linear(x, w_hi, w_lo, inv, None, -1.0, False, None, x, 0)
    assert torch.equal(x, keep)                                     # refused before anything was launched


def test_activation_range():
    rows, K, Nout = 130, 96, 35
    g = torch.Generator().manual_seed(5)
    # up to 6e4: general values inside f16's range keep their 22 bits (the gate is relative: torch's error grows with the values)
    x = torch.randn(rows, K, generator=g)
    check(R.make_case(rows, K, Nout, x=x * (6e4 / float(x.abs().max()))), None, False, True, what="activations up to 6e4")
    # 1e5: hi saturates at 65504 and lo takes the rest
    x = 1e3 * torch.randn(rows, K, generator=g)
    x[torch.rand(rows, K, generator=g) < 0.2] = 1e5
    x[torch.rand(rows, K, generator=g) < 0.2] = -1e5
    got = check(R.make_case(rows, K, Nout, x=x), None, False, True, what="activations of 1e5")
    assert bool(torch.isfinite(got).all())
    # 1e-30: lo is subnormal or zero, hi is zero; beside ordinary values and as a whole row
    x = torch.randn(rows, K, generator=g)
    tiny = 1e-30 * torch.randn(rows, K, generator=g)
    m = torch.rand(rows, K, generator=g) < 0.5
    x[m] = tiny[m]
    x[7] = tiny[7]
    for norm_eps, gelu in ((None, False), (None, True), (U.EPS, True)):
        check(R.make_case(rows, K, Nout, x=x), norm_eps, gelu, True, what=f"activations of 1e-30 (LN {norm_eps is not None})")
    # a constant row under the LayerNorm: variance 0, the row is act(bias), the same as a row of zeros without it
    c = R.make_case(rows, K, Nout)
    c["x"][3], c["x"][129] = 1.5, -3.0                              # sums of these are exact: the mean is the constant
    got = check(c, U.EPS, True, False, what="constant rows under the LayerNorm")
    zero = uf().rows_linear(torch.zeros(1, K, device=DEV), R.linear_module(c["W"], c["b"], DEV), gelu=True)
    assert torch.equal(got[3], zero[0]) and torch.equal(got[129], zero[0])


def test_a_non_finite_value_stays_in_its_row_or_column():
    rows, K, Nout = 130, 40, 35
    c = R.make_case(rows, K, Nout)
    c["W"][0, 0] = 0.9                                              # the largest weight stays where it is: one scale for every call
    lin = R.linear_module(c["W"], c["b"], DEV)
    res = c["res"].to(DEV)
    for norm_eps, gelu in ((None, False), (U.EPS, True)):
        clean = uf().rows_linear(c["x"].to(DEV), lin, norm_eps=norm_eps, gelu=gelu, residual=res)
        x = c["x"].clone()
        x[5, 3], x[70, 0], x[129, 39] = float("nan"), float("inf"), float("-inf")
        got = uf().rows_linear(x.to(DEV), lin, norm_eps=norm_eps, gelu=gelu, residual=res)
        others = torch.ones(rows, dtype=torch.bool)
        others[[5, 70, 129]] = False
        assert torch.equal(got[others], clean[others]) and bool(torch.isfinite(clean).all())
        assert bool(torch.isnan(got[5]).all()) and not torch.equal(got[70], clean[70]) and not torch.equal(got[129], clean[129])
        W = c["W"].clone()
        W[7, 2], W[33, 39] = float("nan"), float("inf")
        got = uf().rows_linear(c["x"].to(DEV), R.linear_module(W, c["b"], DEV), norm_eps=norm_eps, gelu=gelu, residual=res)
        others = torch.ones(Nout, dtype=torch.bool)
        others[[7, 33]] = False
        assert torch.equal(got[:, others], clean[:, others])
        assert bool(torch.isnan(got[:, 7]).all()) and not bool(torch.isfinite(got[:, 33]).all())


def test_zero_weights_give_the_bias_through_the_activation():
    rows, K, Nout = 130, 96, 35
    c = R.make_case(rows, K, Nout, W=torch.zeros(Nout, K))
    lin = R.linear_module(c["W"], c["b"], DEV)
    x, res, b = c["x"].to(DEV), c["res"].to(DEV), c["b"].to(DEV)
    for precision in ("f16x3", "f16"):
        assert torch.equal(uf().rows_linear(x, lin, norm_eps=U.EPS, residual=res, precision=precision), res + b)      # exactly
        assert torch.equal(uf().rows_linear(x, lin, precision=precision), b.expand(rows, Nout))
        got = uf().rows_linear(x, lin, gelu=True, precision=precision)
        assert torch.equal(got, got[:1].expand(rows, Nout))                                                         # one value a column
        gelu64 = torch.nn.functional.gelu(c["b"].double(), approximate="tanh")
        assert float((got[0].cpu().double() - gelu64).abs().max()) <= 4 * 2.0 ** -24 * float(gelu64.abs().max() + 1)  # a few ulp of tanh
        assert torch.equal(uf().rows_linear(x, lin, gelu=True, residual=res, precision=precision), res + got)
    assert math.isclose(uf().pack_linear(lin.weight)[2], 1.0)
