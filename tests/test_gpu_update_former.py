"""GPU half of the update transformer (batrack_amd/frontend/update_former.py over batrack_amd/csrc/attention.hip): the
reference's fixture cases through `forward` on a module tree with timm's attribute names, within twice the larger of the
reference's own float32 error (the gate) and the error of the float32 restatement on the same GPU (the device's float32 GEMMs
sum in another order than the CPU's); the refusals; install()."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import update_former_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = dict(np.load(U.GOLD))


def uf():
    from batrack_amd.frontend import update_former
    return update_former


@pytest.mark.parametrize("c", list(U.CASES))
def test_fixture_cases_through_forward(c):
    spec = U.CASES[c]
    T = U.case_tensors(c, device=DEV)
    out64 = torch.from_numpy(D[f"{c}.out64"]).to(DEV)
    got = uf().forward(U.module_tree(T, spec), T["x"])
    assert got.shape == (1, spec["N"], spec["S"], U.OUTPUT_DIM) and got.dtype == torch.float32 and got.is_contiguous()
    gate = float(D[f"{c}.gate"])
    e_gpu = float((U.transformer(T, spec).double() - out64).abs().max())
    err = float((got.double() - out64).abs().max())
    print(f"case {c}: max |forward - out64| {err:.3e}, gate {gate:.3e}, float32 restatement on the GPU {e_gpu:.3e}")
    assert err <= 2 * max(gate, e_gpu), (c, err, gate, e_gpu)
    # one block alone, both axes
    x = torch.randn(spec["N"] * spec["S"], U.HIDDEN, generator=torch.Generator().manual_seed(3)).to(DEV)
    for axis, p in (("time", "time_blocks.0."), ("space", "space_blocks.0.")):
        blk = getattr(U.module_tree(T, spec), p.split(".")[0])[0]
        y = uf().attn_block(x, blk, axis, spec["N"], spec["S"])
        T64 = {k: v.double() for k, v in T.items()}
        truth = U.block(x.double(), T64, p, axis, spec["N"], spec["S"])
        e_ref = float((U.block(x, T, p, axis, spec["N"], spec["S"]).double() - truth).abs().max())
        e = float((y.double() - truth).abs().max())
        print(f"case {c} one {axis} block: max |attn_block - f64| {e:.3e}, float32 restatement {e_ref:.3e}")
        assert y.shape == x.shape and e <= 2 * e_ref


def test_refusals():
    spec = U.CASES["a"]
    T = U.case_tensors("a", device=DEV)
    ok = lambda: U.module_tree(T, spec)
    with pytest.raises(RuntimeError, match="heads of 48"):
        uf().forward(U.module_tree(T, spec, heads=3), T["x"])                      # heads of 32
    m = ok()
    m.space_blocks[1].attn.q_norm = nn.LayerNorm(U.HEAD_DIM).to(DEV)
    with pytest.raises(RuntimeError, match="q_norm"):
        uf().forward(m, T["x"])
    m = ok()
    m.time_blocks[0].attn.k_norm = nn.LayerNorm(U.HEAD_DIM).to(DEV)
    with pytest.raises(RuntimeError, match="k_norm"):
        uf().forward(m, T["x"])
    m = ok()
    m.time_blocks[1].attn.attn_drop = nn.Dropout(0.1)
    assert uf().forward(m, T["x"]).shape[0] == 1                                   # evaluation mode: dropout is the identity
    with pytest.raises(RuntimeError, match="dropout"):
        uf().forward(m.train(), T["x"])
    with pytest.raises(RuntimeError, match="B = 1"):
        uf().forward(ok(), torch.cat([T["x"], T["x"]], 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        uf().forward(ok(), T["x"].cpu())


def test_install_on_a_stand_in_module_goes_through_the_kernel():
    spec = U.CASES["b"]
    T = U.case_tensors("b", device=DEV)
    mod = types.ModuleType("stand_in_blocks")

    class UpdateFormer(U.Tree):
        def forward(self, input_tensor):
            raise AssertionError("the stand-in's own forward must not run once installed")
    mod.UpdateFormer = UpdateFormer
    previous = uf().install(mod)
    assert previous is not uf().forward and mod.UpdateFormer.forward is uf().forward
    model = U.module_tree(T, spec, cls=mod.UpdateFormer)
    seen = []
    real = uf().attention
    uf().attention = lambda *a, **k: seen.append(a[2:6]) or real(*a, **k)
    try:
        got = model(T["x"])
    finally:
        uf().attention = real
    N, S = spec["N"], spec["S"]
    assert seen == [(N, S, S, 1), (S, N, 1, S), (N, S, S, 1), (N, S, S, 1), (S, N, 1, S), (N, S, S, 1)]    # the every-other interleave
    assert torch.equal(got, uf().forward(U.module_tree(T, spec), T["x"]))
