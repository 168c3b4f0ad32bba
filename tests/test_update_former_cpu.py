"""CPU half of the update transformer (include/batrack_attn.h, batrack_amd/frontend/update_former.py): the reference's fixture
(tests/golden/update_former.npz, made by its unmodified UpdateFormer on a restated timm) against the row-wise restatement of
tests/update_former_util.py; the index specification of bt_attention (gather == rearrange, bit for bit); the digests, the
signature, install(), the wiring, the ABI's refusals and the refusal of CPU tensors — none of which touch a GPU."""
import ctypes
import inspect
import os
import types

import numpy as np
import pytest
import torch

import update_former_util as U
from batrack_amd import _lib

D = dict(np.load(U.GOLD))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c", list(U.CASES))
def test_restatement_reproduces_the_reference(c):
    spec = U.CASES[c]
    out64 = torch.from_numpy(D[f"{c}.out64"])
    got64 = U.transformer(U.case_tensors(c, torch.float64), spec)
    e64 = float((got64 - out64).abs().max())
    got32 = U.transformer(U.case_tensors(c, torch.float32), spec)
    gate = float(D[f"{c}.gate"])
    e32 = float((got32.double() - torch.from_numpy(D[f"{c}.out32"]).double()).abs().max())
    print(f"case {c}: float64 restatement - out64 {e64:.3e}; float32 restatement - out32 {e32:.3e}, gate {gate:.3e}")
    assert got64.shape == out64.shape == (1, spec["N"], spec["S"], U.OUTPUT_DIM)
    assert e64 <= 1e-12
    assert 0 < gate < 1e-4 and gate == float((torch.from_numpy(D[f"{c}.out32"]).double() - out64).abs().max())
    assert got32.dtype == torch.float32 and e32 <= gate


@pytest.mark.parametrize("c", list(U.CASES))
def test_generator_reproduces_the_fixtures_inputs(c):
    d = U.make_inputs(**U.CASES[c])
    names = [n + s for n, _, _ in U.linear_names(U.CASES[c]["time_depth"], U.CASES[c]["space_depth"]) for s in (".weight", ".bias")] + ["x"]
    assert sorted(d) == sorted(names)
    for name in names:
        assert np.array_equal(U.digest(d[name]), D[f"{c}.digest.{name}"]), name
        assert np.array_equal(d[name], d[name].astype(np.float32).astype(np.float64))          # float32 values
        assert np.abs(d[name]).min() > 0 or name == "x"                                        # non-zero biases


def test_fixture_cases_cover_what_they_claim():
    sp = U.CASES
    assert [(s["time_depth"], s["space_depth"], s["N"], s["S"]) for s in sp.values()] == [(2, 2, 37, 12), (4, 2, 70, 5), (2, 1, 130, 12)]
    assert (U.HIDDEN, U.HEADS, U.HEAD_DIM, U.INPUT_DIM, U.OUTPUT_DIM) == (96, 2, 48, 40, 19)
    assert os.path.getsize(U.GOLD) < 600 * 1024


@pytest.mark.parametrize("N,S", [(37, 12), (5, 3), (1, 7), (130, 2)])
def test_gather_is_the_rearranged_attention(N, S):
    """The row index b * seq_stride + i * tok_stride with the two axes' strides is the reference's rearrange / permute:
    bit for bit in float64, with padding columns in the rows."""
    g = torch.Generator().manual_seed(N * 100 + S)
    qkv = torch.randn(N * S, 3 * U.HIDDEN + 5, generator=g, dtype=torch.float64)
    t = U.attention_gather(qkv, U.HEADS, N, S, S, 1)
    s = U.attention_gather(qkv, U.HEADS, S, N, 1, S)
    assert torch.equal(t, U.attention_rearranged(qkv, U.HEADS, N, S, "time"))
    assert torch.equal(s, U.attention_rearranged(qkv, U.HEADS, N, S, "space"))
    assert N == 1 or S == 1 or not torch.equal(t, s)


def test_signature_is_the_references():
    from batrack_amd.frontend import update_former
    got = str(inspect.signature(update_former.forward))
    assert [got] == list(D["signatures"]) and got == "(self, input_tensor)"


def test_install_returns_the_previous_binding_and_is_idempotent():
    from batrack_amd.frontend import update_former
    mod = types.ModuleType("stand_in_blocks")
    old = lambda self, input_tensor: None
    mod.UpdateFormer = type("UpdateFormer", (), {"forward": old})
    assert update_former.install(mod) is old
    assert mod.UpdateFormer.forward is update_former.forward
    assert update_former.install(mod) is update_former.forward
    assert mod.UpdateFormer.forward is update_former.forward


def test_symbol_is_exported_and_sources_listed():
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "batrack_attn.h")).read()
    assert hasattr(L, "bt_attention") and "int bt_attention(" in header and "#define BT_ATTN_HEAD_DIM 48" in header
    assert "attention.hip" in _lib.SOURCES
    assert any(h.endswith("batrack_attn.h") for h in _lib.HEADERS)
    assert "attention" in _lib.ERRORS[_lib.BT_EUNSUPPORTED]
    assert "batrack_attn.h" in open(os.path.join(ROOT, "include", "batrack_track.h")).read()
    import batrack_amd.frontend
    assert "update_former" in batrack_amd.frontend.__doc__
    ops = _lib.torch_ops(strict=True)
    assert str(ops.attention.default._schema) == (
        "batrack_hip::attention(Tensor qkv, int heads, int n_seq, int L, int seq_stride, int tok_stride, float scale) -> Tensor")


def test_abi_refuses_before_launching():
    """Argument checks return their codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    p = ctypes.c_void_p(256)                           # never dereferenced: every call below is refused first or has n_seq == 0
    f = ctypes.c_float
    EINVAL, EUNS, OK = _lib.BT_EINVAL, _lib.BT_EUNSUPPORTED, _lib.BT_OK
    ok = dict(qkv=p, qs=1152, out=p, os=384, n_seq=0, L=12, seq_stride=12, tok_stride=1, heads=8, hd=48, scale=f(48 ** -0.5))
    at = lambda **k: L.bt_attention(*(dict(ok, **k)[n] for n in ok), None)
    assert at() == OK and at(L=1536, seq_stride=1, tok_stride=12) == OK and at(qs=1159, os=389) == OK
    for k in (dict(qkv=None), dict(out=None), dict(n_seq=-1), dict(L=0), dict(heads=0), dict(hd=0), dict(hd=-48), dict(qs=1151), dict(os=383),
              dict(seq_stride=0), dict(tok_stride=0), dict(scale=f(float("nan"))), dict(scale=f(float("inf"))), dict(scale=f(float("-inf"))),
              dict(heads=1 << 62), dict(n_seq=7, L=0), dict(n_seq=7, qs=0)):
        assert at(**k) == EINVAL, k
    M = (1 << 31) - 1
    for k in (dict(hd=32, qs=2000), dict(hd=64, qs=1536, os=512), dict(n_seq=M + 1), dict(L=M - 127), dict(seq_stride=M + 1),
              dict(tok_stride=M + 1), dict(qs=M + 1), dict(os=M + 1),
              dict(n_seq=1 << 20, seq_stride=1 << 12),                                  # the largest row index
              dict(n_seq=2, L=1 << 20, seq_stride=1, tok_stride=1 << 12),
              dict(n_seq=1 << 23, seq_stride=12),                                       # short path: 2^24 workgroups
              dict(n_seq=1 << 11, L=1 << 13, seq_stride=1 << 13, heads=128, qs=3 * 128 * 48, os=128 * 48)):   # long path: 2^24
        assert at(**k) == EUNS, k
    assert at(hd=64, qs=100) == EINVAL                 # a row too narrow for its columns is invalid whatever the head size


def test_cpu_tensors_raise():
    from batrack_amd.frontend import update_former
    T = U.case_tensors("a")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        update_former.attention(torch.zeros(24, 3 * U.HIDDEN), U.HEADS, 2, 12, 12, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        update_former.forward(U.module_tree(T, U.CASES["a"]), T["x"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        update_former.attn_block(torch.zeros(24, U.HIDDEN), U.module_tree(T, U.CASES["a"]).time_blocks[0], "time", 2, 12)
    ops = _lib.torch_ops(strict=True)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.attention(torch.zeros(24, 3 * U.HIDDEN), U.HEADS, 2, 12, 12, 1, 0.1)
