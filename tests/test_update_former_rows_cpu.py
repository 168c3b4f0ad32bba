"""CPU half of the fused transformer rows (include/batrack_rows.h, batrack_amd/frontend/update_former.py): pack_linear against
its specification, the f16 x 3 emulation of tests/rows_util.py on the fixture's cases, the exported symbol and the wiring,
install(precision=None), every refusal of the Python layer and of the ABI — none of which touch a GPU."""
import ctypes
import inspect
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import rows_util as R
import update_former_util as U
from batrack_amd import _lib
from batrack_amd.frontend import update_former

D = dict(np.load(U.GOLD))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape,mag", [((19, 96), 1.0), ((96, 40), 0.11), ((384, 96), 3.7), ((8, 8), 1e-3), ((5, 16), 250.0)])
def test_pack_linear_meets_its_specification(shape, mag):
    W = mag * torch.randn(shape, generator=torch.Generator().manual_seed(shape[0]))
    hi, lo, inv = update_former.pack_linear(W)
    s = 1.0 / inv
    assert hi.dtype == lo.dtype == torch.float16 and hi.shape == lo.shape == W.shape and hi.is_contiguous() and lo.is_contiguous()
    assert s == 2.0 ** round(np.log2(s)) and 2.0 ** -14 <= s <= 2.0 ** 14                          # a power of two inside the clamp
    m = float(W.abs().max())
    assert s == 2.0 ** np.floor(np.log2(1.0 / m)) and 0.5 < m * s <= 1.0
    ws = W * s                                                                                     # exact: a power of two
    assert torch.equal(hi, ws.half()) and torch.equal(lo, (ws - ws.half().float()).half())        # the two rounding statements
    r_hi, r_lo, r_inv = R.pack(W)                                                                  # and the tests' own emulation
    assert torch.equal(hi, r_hi) and torch.equal(lo, r_lo) and inv == r_inv
    rebuilt = (hi.double() + lo.double()) * inv
    assert float((rebuilt - W.double()).abs().max()) <= 2.0 ** -22 * m * 2                         # 22 bits of the largest entry


def test_pack_linear_scale_edges():
    hi, lo, inv = update_former.pack_linear(torch.zeros(7, 16))
    assert inv == 1.0 and not hi.any() and not lo.any()                                            # all-zero: s = 1
    W = torch.randn(4, 8, generator=torch.Generator().manual_seed(1))
    assert update_former.pack_linear(1e-20 * W)[2] == 2.0 ** -14                                   # s clamped to 2^14
    assert update_former.pack_linear(1e20 * W)[2] == 2.0 ** 14                                     # s clamped to 2^-14
    assert update_former.pack_linear(torch.full((2, 8), 0.5))[2] == 0.5                            # 1 / max is a power of two: s = 2
    assert update_former.pack_linear(torch.full((2, 8), 0.75))[2] == 1.0
    Wn = W.clone()
    Wn[1, 3], Wn[2, 0] = float("nan"), float("inf")                                                # the scale is taken over the finite entries
    h, l, inv = update_former.pack_linear(Wn)
    Wf = W.clone()
    Wf[1, 3] = Wf[2, 0] = 0
    assert inv == update_former.pack_linear(Wf)[2]
    assert torch.isnan(h[1, 3]) and torch.isinf(h[2, 0]) and torch.isfinite(h[0]).all() and torch.isfinite(h[3]).all()
    with pytest.raises(RuntimeError, match=r"\[Nout, K\]"):
        update_former.pack_linear(torch.zeros(8))


@pytest.mark.parametrize("c", list(U.CASES))
def test_f16x3_emulation_of_the_transformer_is_float32_grade(c):
    """Measured: 0.79 / 0.86 / 1.19 x the fixture's gate on cases a / b / c; held to twice the gate, as update_former.forward is.
    One f16 product alone is about 1000 x the gate: the cross terms are what carries the accuracy."""
    spec = U.CASES[c]
    T = U.case_tensors(c, torch.float32)
    out64 = torch.from_numpy(D[f"{c}.out64"])
    gate = float(D[f"{c}.gate"])
    e3 = float((R.emu_transformer(T, spec, "f16x3").double() - out64).abs().max())
    e1 = float((R.emu_transformer(T, spec, "f16").double() - out64).abs().max())
    print(f"case {c}: f16x3 emulation - out64 {e3:.3e} = {e3 / gate:.2f} x gate {gate:.3e}; f16 alone {e1:.3e} = {e1 / gate:.0f} x")
    assert e3 <= 2 * gate
    assert e1 > 50 * gate


def test_symbol_is_exported_and_sources_listed():
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "batrack_rows.h")).read()
    assert hasattr(L, "bt_rows_linear") and "int bt_rows_linear(" in header and "#define BT_ROWS_TILE 128" in header
    assert "rows_linear.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "rows_linear.hip"))
    assert any(h.endswith("batrack_rows.h") for h in _lib.HEADERS)
    assert "rows_linear" in _lib.ERRORS[_lib.BT_EUNSUPPORTED]
    assert _lib.BT_ROWS_PRECISION == {"f16x3": 0, "f16": 1} and "BT_ROWS_F16X3 = 0, BT_ROWS_F16 = 1" in header
    ops = _lib.torch_ops(strict=True)
    assert str(ops.rows_linear.default._schema) == (
        "batrack_hip::rows_linear(Tensor x, Tensor w_hi, Tensor w_lo, float inv_scale, Tensor? bias, float norm_eps, bool gelu, "
        "Tensor? residual, Tensor(a!) out, int precision) -> ()")
    assert str(inspect.signature(update_former.rows_linear)) == (
        "(x, lin, *, norm_eps=None, gelu=False, residual=None, out=None, precision='f16x3')")
    assert str(inspect.signature(update_former.attn_block_rows)) == "(x, blk, axis, N, S, precision='f16x3')"
    assert str(inspect.signature(update_former.forward_rows)) == "(self, input_tensor, precision='f16x3')"
    assert str(inspect.signature(update_former.install)) == "(module=None, precision=None)"


def test_install_binds_forward_or_forward_rows():
    mod = types.ModuleType("stand_in_blocks")
    old = lambda self, input_tensor: None
    mod.UpdateFormer = type("UpdateFormer", (), {"forward": old})
    assert update_former.install(mod, precision=None) is old
    assert mod.UpdateFormer.forward is update_former.forward                    # None: exactly the binding of before
    for p in ("f16x3", "f16"):
        previous = update_former.install(mod, precision=p)
        bound = mod.UpdateFormer.forward
        assert previous is not None and bound is not update_former.forward and bound.precision == p
        assert list(inspect.signature(bound).parameters) == ["self", "input_tensor"]      # called as a module: one argument
    assert update_former.install(mod) is bound and mod.UpdateFormer.forward is update_former.forward
    with pytest.raises(RuntimeError, match="unknown precision"):
        update_former.install(mod, precision="bf16")
    assert mod.UpdateFormer.forward is update_former.forward                    # a refused install changes nothing


def test_every_refusal_names_its_reason():
    """The checks run before any tensor is touched on a device, so CPU modules show them; the last check is the CPU tensor's."""
    spec = U.CASES["a"]
    T = U.case_tensors("a")
    ok = lambda **k: U.module_tree(T, spec, **k)
    fr = update_former.forward_rows

    class OnGpu(torch.Tensor):                         # passes `_gpu` without a GPU; nothing below reaches a kernel
        is_cuda = True
    x = T["x"].as_subclass(OnGpu)
    m = ok()
    m.time_blocks[1].norm1 = nn.LayerNorm(U.HIDDEN, eps=U.EPS)
    with pytest.raises(RuntimeError, match="norm1 has affine parameters"):
        fr(m, x)
    m = ok()
    m.space_blocks[0].norm2 = nn.LayerNorm(U.HIDDEN, eps=U.EPS)
    with pytest.raises(RuntimeError, match="norm2 has affine parameters"):
        fr(m, x)
    for act in (nn.GELU(), nn.ReLU()):
        m = ok()
        m.time_blocks[0].mlp.act = act
        with pytest.raises(RuntimeError, match="approximate='tanh'"):
            fr(m, x)
    for name in ("q_norm", "k_norm"):
        m = ok()
        setattr(m.space_blocks[1].attn, name, nn.LayerNorm(U.HEAD_DIM))
        with pytest.raises(RuntimeError, match=name):
            fr(m, x)
    m = ok()
    m.time_blocks[1].mlp.drop1 = nn.Dropout(0.1)
    with pytest.raises(RuntimeError, match="dropout"):
        fr(m.train(), x)
    with pytest.raises(RuntimeError, match="B = 1"):
        fr(ok(), torch.cat([T["x"], T["x"]], 0).as_subclass(OnGpu))
    with pytest.raises(RuntimeError, match="heads of 48"):
        fr(ok(heads=3), x)
    for f in (lambda: fr(ok(), x, precision="bf16x3"), lambda: update_former.attn_block_rows(x[0].reshape(-1, U.INPUT_DIM), None, "time", 37, 12, "f32"),
              lambda: update_former.rows_linear(x, None, precision="f16x2")):
        with pytest.raises(RuntimeError, match="unknown precision"):
            f()
    blk = ok().time_blocks[0]
    with pytest.raises(RuntimeError, match="axis must be"):
        update_former.attn_block_rows(torch.zeros(24, U.HIDDEN).as_subclass(OnGpu), blk, "depth", 2, 12)
    with pytest.raises(RuntimeError, match="affine"):
        blk.norm1 = nn.LayerNorm(U.HIDDEN)
        update_former.attn_block_rows(torch.zeros(24, U.HIDDEN).as_subclass(OnGpu), blk, "time", 2, 12)
    for f in (lambda: fr(ok(), T["x"]), lambda: update_former.rows_linear(torch.zeros(4, U.HIDDEN), ok().flow_head),
              lambda: update_former.attn_block_rows(torch.zeros(24, U.HIDDEN), ok().time_blocks[0], "time", 2, 12)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()


def test_abi_refuses_before_launching():
    """Argument checks return their codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    p, q, w = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 12)     # never dereferenced
    f = ctypes.c_float
    EINVAL, EUNS, OK = _lib.BT_EINVAL, _lib.BT_EUNSUPPORTED, _lib.BT_OK
    ok = dict(x=p, ldx=96, w_hi=w, w_lo=w, inv=f(1.0), bias=None, res=None, ldr=0, out=q, ldo=19, rows=0, K=96, Nout=19, pro=1, eps=f(1e-6),
              act=1, prec=0)
    rl = lambda **k: L.bt_rows_linear(*(dict(ok, **k)[n] for n in ok), None)
    assert rl() == OK and rl(pro=0, act=0, prec=1, ldx=100, ldo=24) == OK
    for k in (dict(x=None), dict(w_hi=None), dict(w_lo=None), dict(out=None), dict(rows=-1), dict(Nout=0), dict(K=0), dict(K=12, ldx=12),
              dict(K=4, ldx=4), dict(K=100, ldx=100), dict(ldx=95), dict(ldo=18), dict(res=q, ldr=18), dict(pro=2), dict(act=2), dict(prec=2),
              dict(prec=-1), dict(inv=f(0.0)), dict(inv=f(-1.0)), dict(inv=f(float("nan"))), dict(inv=f(float("inf"))),
              dict(eps=f(-1e-6)), dict(eps=f(float("nan")))):
        assert rl(**k) == EINVAL, k
    assert rl(pro=0, eps=f(-1.0)) == OK                                    # eps is read with the LayerNorm only
    M = (1 << 31) - 1
    for k in (dict(rows=M + 1), dict(K=M + 1, ldx=M + 1), dict(Nout=M + 1, ldo=M + 1), dict(ldx=M + 1), dict(ldo=M + 1),
              dict(res=q, ldr=M + 1), dict(rows=M, Nout=M, ldo=M)):
        assert rl(**k) == EUNS, k
    # overlap: checked once there are rows, still before any launch
    assert rl(rows=4, out=p) == EINVAL                                                           # out is x
    assert rl(rows=4, out=ctypes.c_void_p((1 << 20) + 4 * (3 * 96 + 95))) == EINVAL              # out starts on the last element of x
    assert rl(rows=4, res=ctypes.c_void_p((1 << 30) + 4), ldr=19) == EINVAL                      # a residual shifted against out
    assert rl(rows=4, res=q, ldr=20) == EINVAL                                                   # the same start, another stride
