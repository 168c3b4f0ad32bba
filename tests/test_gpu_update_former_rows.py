"""GPU half of the fused transformer rows (batrack_amd/csrc/rows_linear.hip through update_former.rows_linear,
attn_block_rows, forward_rows): every prologue / epilogue / residual combination at the fixture's shapes against the same
statement in float64, gated by twice the error torch's float32 run of that statement makes ("f16x3") or twice the error of the
hi-only emulation ("f16"); row independence and repeatability bit for bit; the fixture's cases through forward_rows; install()."""
import itertools
import types

import numpy as np
import pytest
import torch

import rows_util as R
import update_former_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = dict(np.load(U.GOLD))
ROWS = 37 * 12
COMBOS = list(itertools.product((None, U.EPS), (False, True), (False, True)))          # LayerNorm x GELU x residual


def uf():
    from batrack_amd.frontend import update_former
    return update_former


def call(c, lin, norm_eps, gelu, residual, precision, **k):
    res = c["res"].to(DEV) if residual else None
    return uf().rows_linear(c["x"].to(DEV), lin, norm_eps=norm_eps, gelu=gelu, residual=res, precision=precision, **k)


@pytest.mark.parametrize("K,Nout", list(itertools.product((40, 96, 384), (19, 96, 288, 384))))
def test_rows_linear_against_float64(K, Nout):
    c = R.make_case(ROWS, K, Nout)
    lin = R.linear_module(c["W"], c["b"], DEV)
    for precision in ("f16x3", "f16"):
        for norm_eps, gelu, residual in COMBOS:
            truth, gate = R.gates(c, norm_eps, gelu, residual, precision)
            got = call(c, lin, norm_eps, gelu, residual, precision)
            assert got.shape == (ROWS, Nout) and got.dtype == torch.float32 and got.is_contiguous()
            err = float((got.cpu().double() - truth).abs().max())
            print(f"K {K} Nout {Nout} {precision} LN {norm_eps is not None} GELU {gelu} residual {residual}: "
                  f"max |rows_linear - f64| {err:.3e} = {2 * err / gate:.2f} x the reference's error (gate: 2 x)")
            assert err <= gate, (precision, norm_eps, gelu, residual, err, gate)
    nb = R.make_case(ROWS, K, Nout, bias=False)                                         # a Linear without a bias
    truth, gate = R.gates(nb, U.EPS, True, True, "f16x3")
    assert float((call(nb, R.linear_module(nb["W"], None, DEV), U.EPS, True, True, "f16x3").cpu().double() - truth).abs().max()) <= gate


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_rows_do_not_depend_on_their_place_and_calls_repeat(precision):
    c = R.make_case(ROWS, 96, 288)
    c["W"][150, 3] = 0.9                                                                # the largest weight: the slice below shares the scale
    lin = R.linear_module(c["W"], c["b"], DEV)
    x, res = c["x"].to(DEV), c["res"].to(DEV)
    for norm_eps, gelu in ((None, False), (U.EPS, True)):
        full = uf().rows_linear(x, lin, norm_eps=norm_eps, gelu=gelu, residual=res, precision=precision)
        assert torch.equal(full, uf().rows_linear(x, lin, norm_eps=norm_eps, gelu=gelu, residual=res, precision=precision))
        for a, b in ((0, 1), (5, 133), (127, 129), (130, 444), (301, 302)):            # other tiles, other places in a tile
            part = uf().rows_linear(x[a:b], lin, norm_eps=norm_eps, gelu=gelu, residual=res[a:b], precision=precision)
            assert torch.equal(part, full[a:b]), (norm_eps, gelu, a, b)
    # a saturating activation (|a| > 65488: the fourth product) in one row leaves the other rows of its tile as they are,
    # whether the workgroup takes the extra step for that K step or skips it: row 3 in the first tile, K step 1; row 200 in the
    # second, K step 2; compared with the call that has neither
    hot = x.clone()
    hot[3, 40], hot[200, 70] = 1e5, -7e4
    others = torch.ones(ROWS, dtype=torch.bool, device=DEV)
    others[[3, 200]] = False
    for norm_eps, gelu in ((None, False), (None, True)):
        full = uf().rows_linear(x, lin, norm_eps=norm_eps, gelu=gelu, residual=res, precision=precision)
        got = uf().rows_linear(hot, lin, norm_eps=norm_eps, gelu=gelu, residual=res, precision=precision)
        assert torch.equal(got[others], full[others]) and not torch.equal(got[3], full[3]) and not torch.equal(got[200], full[200])
        assert torch.equal(got[3:4], uf().rows_linear(hot[3:4], lin, norm_eps=norm_eps, gelu=gelu, residual=res[3:4], precision=precision))
    # a column's arithmetic does not depend on its place either: the Linear of a slice of W's rows
    sub = R.linear_module(c["W"][100:231], c["b"][100:231], DEV)
    assert torch.equal(uf().rows_linear(x, sub, norm_eps=U.EPS, gelu=True, precision=precision),
                       uf().rows_linear(x, lin, norm_eps=U.EPS, gelu=True, precision=precision)[:, 100:231])


@pytest.mark.parametrize("c", list(U.CASES))
def test_fixture_cases_through_forward_rows(c):
    spec = U.CASES[c]
    T = U.case_tensors(c, device=DEV)
    out64 = torch.from_numpy(D[f"{c}.out64"])
    gate = float(D[f"{c}.gate"])
    model = U.module_tree(T, spec)
    got = uf().forward_rows(model, T["x"])
    assert got.shape == (1, spec["N"], spec["S"], U.OUTPUT_DIM) and got.dtype == torch.float32 and got.is_contiguous()
    err = float((got.cpu().double() - out64).abs().max())
    print(f"case {c}: max |forward_rows(f16x3) - out64| {err:.3e} = {err / gate:.2f} x gate {gate:.3e} (held to 2 x)")
    assert err <= 2 * gate, (c, err, gate)
    assert torch.equal(got, uf().forward_rows(model, T["x"], precision="f16x3"))
    # one f16 product: within twice the error of its emulation
    e_emu = float((R.emu_transformer(U.case_tensors(c), spec, "f16").double() - out64).abs().max())
    e16 = float((uf().forward_rows(model, T["x"], precision="f16").cpu().double() - out64).abs().max())
    print(f"case {c}: max |forward_rows(f16) - out64| {e16:.3e}, emulation {e_emu:.3e}")
    assert e16 <= 2 * e_emu and e16 > 2 * gate                                          # and it really is the cheaper path
    # one block alone, both axes, against the float64 restatement
    x = torch.randn(spec["N"] * spec["S"], U.HIDDEN, generator=torch.Generator().manual_seed(3))
    T32, T64 = U.case_tensors(c), U.case_tensors(c, torch.float64)
    for axis, p in (("time", "time_blocks.0."), ("space", "space_blocks.0.")):
        blk = getattr(model, p.split(".")[0])[0]
        xd = x.to(DEV)
        y = uf().attn_block_rows(xd, blk, axis, spec["N"], spec["S"])
        truth = U.block(x.double(), T64, p, axis, spec["N"], spec["S"])
        e_ref = float((U.block(x, T32, p, axis, spec["N"], spec["S"]).double() - truth).abs().max())
        e = float((y.cpu().double() - truth).abs().max())
        print(f"case {c} one {axis} block: max |attn_block_rows - f64| {e:.3e}, float32 restatement {e_ref:.3e}")
        assert y.shape == x.shape and e <= 2 * e_ref and torch.equal(xd.cpu(), x)       # x is not written


def test_install_with_a_precision_binds_forward_rows_and_leaves_forward_alone():
    spec = U.CASES["b"]
    T = U.case_tensors("b", device=DEV)
    before = uf().forward(U.module_tree(T, spec), T["x"])
    mod = types.ModuleType("stand_in_blocks")

    class UpdateFormer(U.Tree):
        def forward(self, input_tensor):
            raise AssertionError("the stand-in's own forward must not run once installed")
    mod.UpdateFormer = UpdateFormer
    uf().install(mod, precision="f16x3")
    model = U.module_tree(T, spec, cls=mod.UpdateFormer)
    seen = []
    real = uf().rows_linear
    uf().rows_linear = lambda x, lin, **k: seen.append((lin.weight.shape[0], k["precision"])) or real(x, lin, **k)
    try:
        got = model(T["x"])
    finally:
        uf().rows_linear = real
    blocks = spec["time_depth"] + spec["space_depth"]
    assert [n for n, _ in seen] == [U.HIDDEN] + [3 * U.HIDDEN, U.HIDDEN, U.MLP, U.HIDDEN] * blocks + [U.OUTPUT_DIM]
    assert {p for _, p in seen} == {"f16x3"}
    assert torch.equal(got, uf().forward_rows(U.module_tree(T, spec), T["x"]))
    assert float((got.cpu().double() - torch.from_numpy(D["b.out64"])).abs().max()) <= 2 * float(D["b.gate"])
    assert torch.equal(uf().forward(U.module_tree(T, spec), T["x"]), before)           # `forward` itself is what it was
    assert uf().install(mod) is not uf().forward and mod.UpdateFormer.forward is uf().forward
    assert torch.equal(model(T["x"]), before)


def test_packed_weights_follow_an_in_place_update():
    c = R.make_case(40, 96, 96)
    lin = R.linear_module(c["W"], c["b"], DEV)
    x = c["x"].to(DEV)
    first = uf().rows_linear(x, lin)
    assert torch.equal(first, uf().rows_linear(x, lin))
    with torch.no_grad():
        lin.weight.mul_(-2.0)
        lin.bias.zero_()
    second = uf().rows_linear(x, lin)
    fresh = uf().rows_linear(x, R.linear_module(-2.0 * c["W"], torch.zeros(96), DEV))
    assert torch.equal(second, fresh) and not torch.equal(second, first)


def test_the_ctypes_route_gives_the_same_bits(monkeypatch):
    """Without libbatrack_torch.so rows_linear calls bt_rows_linear through ctypes: the same kernel on the same arguments."""
    from batrack_amd import _lib
    c = R.make_case(130, 40, 19)
    lin = R.linear_module(c["W"], c["b"], DEV)
    wide = torch.zeros(130, 47, device=DEV)
    wide[:, 3:43] = c["x"].to(DEV)
    res = c["res"].to(DEV)
    args = lambda: dict(norm_eps=U.EPS, gelu=True, residual=res.clone())
    want = [uf().rows_linear(wide[:, 3:43], lin, precision=p, **args()) for p in ("f16x3", "f16")]
    plain = uf().rows_linear(c["x"].to(DEV), lin)
    monkeypatch.setattr(_lib, "torch_ops", lambda strict=False: None)
    for p, w in zip(("f16x3", "f16"), want):
        k = args()
        got = uf().rows_linear(wide[:, 3:43], lin, precision=p, out=k["residual"], **k)          # strides, and out is the residual
        assert torch.equal(got, w)
    assert torch.equal(uf().rows_linear(c["x"].to(DEV), lin), plain)                            # no bias-less, no residual: the nulls
    assert uf().rows_linear(c["x"].to(DEV)[:0], lin).shape == (0, 19)
    with pytest.raises(RuntimeError, match="overlaps"):
        uf().rows_linear(wide[:, :40], lin, out=wide[:, 8:27])
