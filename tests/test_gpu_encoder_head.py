"""GPU half of the encoder's head (include/batrack_encoder.h, batrack_amd/frontend/encoder.py) against the reference's fixture
(tests/golden/encoder_head.npz) and the restatement in tests/encoder_head_util.py.  No bound here comes from the kernels
under test: the gates are the reference's own float32-vs-float64 differences, stored in the fixture, or the restatement's,
measured here on the same GPU.  Twice the gate: the kernels and the reference each round their own order of the same sums.

Measured on an MI355X (information, not gates): max |encoder_head - ref32| beside the gate
    s4  4.768e-06  3.527e-06      s8  3.338e-06  3.065e-06      thin  2.861e-06  2.748e-06
    forward 5.761e-06 and the mid shape 5.490e-06 against float64, where torch's float32 run is 7.329e-06 and 9.709e-06 off.
(One fma chain over all 3744 products of conv2 gave 1.407e-05 on s4: the kernels sum in short chains)"""
import ctypes
import types

import numpy as np
import pytest
import torch

import encoder_head_util as U
from batrack_amd import _lib

pytestmark = pytest.mark.gpu

D = dict(np.load(U.GOLD))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def encoder():
    from batrack_amd.frontend import encoder
    return encoder


def raw_call(t, packed, size, out=None, ws=None):
    """bt_encoder_head through ctypes on the current stream; `packed` = (w2_packed, bias2, w3_packed, bias3)."""
    L = _lib.lib()
    F, (h, w) = t["a"].shape[0], size
    if out is None:
        out = torch.empty(F, U.COUT, h, w, device=DEV)
    if ws is None:
        ws = torch.empty((L.bt_encoder_head_workspace_bytes(F, h, w) + 7) // 8, dtype=torch.float64, device=DEV)
    lv = [_lib.EncoderLevel(t[n].data_ptr(), *t[n].shape[1:], *t[n].stride()) for n in U.NAMES]
    rc = L.bt_encoder_head(*(ctypes.byref(v) for v in lv), packed[0].data_ptr(), packed[1].data_ptr(), U.CMID, packed[2].data_ptr(),
                           packed[3].data_ptr(), U.COUT, F, h, w, ws.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.BT_OK, rc
    return out


@pytest.mark.parametrize("c", list(U.CASES))
def test_fixture_case_is_within_twice_the_gate_on_every_route(encoder, c):
    spec, t = U.CASES[c], U.case_tensors(c, device=DEV)
    conv2, conv3 = U.convs(t)
    gate, want = float(D[f"{c}.gate"]), torch.from_numpy(D[f"{c}.out32"])
    got = encoder.encoder_head(*(t[n] for n in U.NAMES), conv2, conv3, spec["size"])
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous()
    err = float((got.cpu().double() - want.double()).abs().max())
    print(f"case {c}: max |encoder_head - ref32| {err:.3e}, gate {gate:.3e}")
    assert 0 < gate < 5e-5 and err <= 2 * gate, (c, err, gate)
    packed = encoder.packed_head(conv2, conv3)
    by_abi = raw_call(t, packed, spec["size"])
    by_op = torch.empty_like(got)
    _lib.torch_ops(strict=True).encoder_head(*(t[n] for n in U.NAMES), *packed, by_op)
    assert torch.equal(by_abi, by_op) and torch.equal(by_abi, got)


def test_forward_on_an_encoder_shaped_module(encoder):
    """A 40 x 72 image through a seeded network of the encoder's shape: 20 x 36, 10 x 18, 5 x 9 and 3 x 5 maps to a 10 x 18
    output.  The bound is the float32 restatement's own error against its float64 run on the same GPU, doubled."""
    m = U.SmallEncoder().to(DEV)
    x = torch.rand(2, 3, 40, 72, generator=torch.Generator().manual_seed(98)).to(DEV) * 2 - 1
    got = encoder.forward(m, x)
    with torch.no_grad():
        want32 = U.encoder_forward(m, x)
        want64 = U.encoder_forward(m.double(), x.double())
    m.float()
    assert got.shape == (2, 128, 10, 18)
    own = float((want32.double() - want64).abs().max())
    err = float((got.double() - want64).abs().max())
    print(f"forward: max |ours - restatement64| {err:.3e}; the float32 restatement's own error {own:.3e}")
    assert 0 < own < 5e-4 and err <= 2 * own

    mod = types.ModuleType("stand_in_blocks")
    mod.BasicEncoder = type("BasicEncoder", (U.SmallEncoder,), {"forward": lambda self, x: None})
    encoder.install(mod)
    m.__class__ = mod.BasicEncoder
    assert mod.BasicEncoder.forward is encoder.forward
    again = m(x)                                                 # (torch's own convolutions need not repeat bit for bit: the bound again)
    err = float((again.double() - want64).abs().max())
    print(f"forward, installed: max |ours - restatement64| {err:.3e}")
    assert again.shape == got.shape and err <= 2 * own


def test_mid_shape_against_the_float64_restatement(encoder):
    """F = 2, a 24 x 32 output (3 x 2 tiles, 6 pixel blocks) from 48 x 64, 24 x 32, 12 x 16 and 6 x 8 maps."""
    size, sizes = (24, 32), ((48, 64), (24, 32), (12, 16), (6, 8))
    t = U.random_tensors(94, 2, sizes, device=DEV)
    conv2, conv3 = U.convs(t)
    got = encoder.encoder_head(*(t[n] for n in U.NAMES), conv2, conv3, size)
    with torch.no_grad():
        want32 = U.head(*(t[n] for n in U.INPUTS), size)
        want64 = U.head(*(t[n].double() for n in U.INPUTS), size)
    own = float((want32.double() - want64).abs().max())
    err = float((got.double() - want64).abs().max())
    print(f"mid shape: max |encoder_head - restatement64| {err:.3e}; the float32 restatement's own error {own:.3e}")
    assert 0 < own < 5e-4 and err <= 2 * own
