"""GPU half of the encoder's stem (bt_encoder_stem in include/batrack_encoder.h, batrack_amd/frontend/encoder.py) against the
reference's fixture (tests/golden/encoder_stem.npz) and the restatement in tests/encoder_stem_util.py.  No bound here comes
from the kernels under test: the gates are the reference's own float32-vs-float64 differences, stored in the fixture, or the
restatement's, measured here on the same GPU.  The comparison is with the FLOAT64 run and the bound is twice the gate.

Measured on an MI355X (information, not gates): max |ours - float64 run| beside the gate
    tiles 7.52e-7 2.47e-6   odd 5.47e-7 1.87e-6   tiny 5.23e-7 1.04e-6
    forward 1.06e-5 with the stem on the kernels and 1.02e-5 with it left to torch, where the float32 restatement on the
    same GPU is 1.2e-5 - 1.4e-5 off (it varies by run).
"""
import numpy as np
import pytest
import torch

import encoder_stem_util as U
import encoder_trunk_util as T
from batrack_amd import _lib

pytestmark = pytest.mark.gpu

D = dict(np.load(U.GOLD))
DEV = "cuda:0"
ROUTES = ("python", "abi", "op")


@pytest.fixture(scope="module")
def encoder():
    from batrack_amd.frontend import encoder
    return encoder


def run_stem(encoder, route, x, conv1):
    if route == "python":
        return encoder.encoder_stem(x, conv1)
    packed = encoder.packed_stem(conv1)
    if route == "abi":
        return U.raw_stem(x, packed)
    out = torch.empty(x.shape[0], U.CSTEM, *U.out_size(x.shape[2:]), device=DEV)
    _lib.torch_ops(strict=True).encoder_stem(x, *packed, out)
    return out


@pytest.mark.parametrize("c", list(U.CASES))
def test_stem_is_within_twice_the_gate_on_every_route(encoder, c):
    t = U.case_tensors(c, device=DEV)
    conv1 = U.conv1_of(t)
    got = {route: run_stem(encoder, route, t["x"], conv1) for route in ROUTES}
    assert tuple(got["python"].shape) == (U.CASES[c]["F"], U.CSTEM, *U.out_size(U.CASES[c]["size"]))
    assert got["python"].dtype == torch.float32 and got["python"].is_contiguous()
    s = got["python"].cpu().numpy().ravel()[::U.STEP[c]].astype(np.float64)
    want, gate = D[f"{c}.out64"], float(D[f"{c}.gate"])
    assert s.shape == want.shape
    err = float(np.abs(s - want).max())
    print(f"case {c}: max |ours - float64 run| {err:.3e}, gate {gate:.3e}")
    assert 0 < gate < 5e-5 and err <= 2 * gate, (c, err, gate)
    assert torch.equal(got["abi"], got["python"]) and torch.equal(got["op"], got["python"])


@pytest.mark.parametrize("flag", [True, False])
def test_forward_with_the_stem_on_and_off(encoder, monkeypatch, flag):
    """A 40 x 72 image through a seeded encoder with real residual layers, `DEVICE_STEM` forced: the bound is the float32
    restatement's own error against its float64 run on the same GPU, doubled."""
    m = T.TrunkEncoder().to(DEV)
    assert encoder.stem_refusal(m) is None
    x = torch.rand(2, 3, 40, 72, generator=torch.Generator().manual_seed(179)).to(DEV) * 2 - 1
    calls = []
    real = encoder.encoder_stem
    monkeypatch.setattr(encoder, "encoder_stem", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(encoder, "DEVICE_STEM", flag)
    got = encoder.forward(m, x)
    assert len(calls) == (1 if flag else 0)
    with torch.no_grad():
        want32 = T.encoder_forward(m, x)
        m.double()
        want64 = T.encoder_forward(m, x.double())
        assert U.conditions_hold([m.conv1(x.double())])
    m.float()
    assert got.shape == (2, 128, 10, 18)
    own = float((want32.double() - want64).abs().max())
    err = float((got.double() - want64).abs().max())
    print(f"forward, DEVICE_STEM {flag}: max |ours - restatement64| {err:.3e}; the float32 restatement's own error {own:.3e}")
    assert 0 < own < 5e-4 and err <= 2 * own
