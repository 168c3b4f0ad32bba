"""CPU half of the encoder's stem (bt_encoder_stem in include/batrack_encoder.h): the reference's fixture
(tests/golden/encoder_stem.npz, made by its unmodified conv1, norm1, relu1) against the torch restatement in
tests/encoder_stem_util.py; the input digests, the weight repack and its cache, `stem_refusal`, `forward`'s choice of path,
the ABI's refusals and the import surface — none of which touch a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import encoder_head_util as H
import encoder_stem_util as U
import encoder_trunk_util as T
from batrack_amd import _lib

D = dict(np.load(U.GOLD))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def encoder():
    from batrack_amd.frontend import encoder
    return encoder


@pytest.fixture(scope="module")
def restated():
    runs = {}
    for c in U.CASES:
        for dtype in (torch.float32, torch.float64):
            t = U.case_tensors(c, dtype)
            runs[c, dtype] = U.stem(t["x"], t["w"], t["b"])
    return runs


@pytest.mark.parametrize("c", list(U.CASES))
def test_generator_reproduces_the_fixtures_inputs(c):
    d = U.make_inputs(**U.CASES[c])
    assert set(d) == set(U.INPUTS)
    for name, v in d.items():
        assert np.array_equal(U.digest(v), D[f"{c}.digest.{name}"]), name
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
    assert np.abs(d["x"]).max() <= 1.0 and d["x"].min() < -0.9 and d["x"].max() > 0.9          # images in +-1
    assert np.abs(d["b"]).max() <= 0.5 and np.abs(d["b"]).sum() > 0                            # uniform in +-0.5, not zero
    assert abs(d["w"].std() / np.sqrt(2.0 / (64 * 49)) - 1) < 0.05                             # kaiming fan-out


@pytest.mark.parametrize("c", list(U.CASES))
def test_float64_restatement_reproduces_the_float64_run(c, restated):
    got, want = restated[c, torch.float64].numpy().ravel()[::U.STEP[c]], D[f"{c}.out64"]
    assert got.shape == want.shape and want.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()


@pytest.mark.parametrize("c", list(U.CASES))
def test_float32_restatement_stays_within_the_gate(c, restated):
    out, gate = restated[c, torch.float32], float(D[f"{c}.gate"])
    assert tuple(out.shape) == (U.CASES[c]["F"], U.CSTEM, *U.out_size(U.CASES[c]["size"]))
    err = float(np.abs(out.numpy().ravel()[::U.STEP[c]].astype(np.float64) - D[f"{c}.out32"]).max())
    print(f"case {c}: max |restatement32 - ref32| {err:.3e}, gate {gate:.3e}")
    assert 0 < gate < 5e-5 and err <= gate


def test_fixture_cases_cover_what_they_claim():
    sizes = {c: U.out_size(U.CASES[c]["size"]) for c in U.CASES}
    assert sizes == dict(tiles=(20, 36), odd=(17, 24), tiny=(4, 3))
    assert [U.CASES[c]["F"] for c in ("tiles", "odd", "tiny")] == [2, 1, 3]
    assert [U.CASES[c]["size"] for c in ("tiles", "odd", "tiny")] == [(40, 72), (33, 47), (7, 5)]
    assert sizes["tiny"][0] * sizes["tiny"][1] == 12                                          # the minimum the condition allows
    for c, (h, w) in sizes.items():
        assert np.gcd(U.STEP[c], w) == 1                                                      # the samples sweep the columns
        t = U.case_tensors(c, torch.float64)
        assert U.conditions_hold([U.raw(t["x"], t["w"], t["b"])]), c
    assert os.path.getsize(U.GOLD) <= os.path.getsize(T.GOLD)


def test_repack_is_a_permutation_plus_zeros(encoder):
    w = U.case_tensors("odd")["w"]
    p = encoder.pack_stem_weights(w)
    assert p.shape == (7, 3, 8, 64) and p.is_contiguous() and p.dtype == torch.float32
    assert torch.equal(p, U.pack_stem_weights(w))
    assert p[2, 1, 5, 60] == w[60, 1, 2, 5] and p[6, 2, 0, 3] == w[3, 2, 6, 0]
    assert float(p[:, :, 7, :].abs().max()) == 0 and int((p == 0).sum()) == 7 * 3 * 64      # the eighth kx, and nothing else
    assert torch.equal(torch.sort(p[:, :, :7, :].flatten())[0], torch.sort(w.flatten())[0])
    for shape in ((64, 4, 7, 7), (32, 3, 7, 7), (64, 3, 3, 3), (64, 3, 7), (64, 3, 7, 5)):
        with pytest.raises(RuntimeError, match="conv1 must be 7 x 7 from 3 to 64"):
            encoder.pack_stem_weights(torch.zeros(shape))


def test_repack_is_cached_on_pointer_and_version(encoder):
    m = U.StemEncoder()
    first = encoder.packed_stem(m.conv1)
    assert all(x is y for x, y in zip(encoder.packed_stem(m.conv1), first))
    assert len(first) == 2 and torch.equal(first[1], m.conv1.bias) and torch.equal(first[0], U.pack_stem_weights(m.conv1.weight))
    with torch.no_grad():
        m.conv1.weight.mul_(2.0)                                  # the version moves
    second = encoder.packed_stem(m.conv1)
    assert second[0] is not first[0] and torch.equal(second[0], first[0] * 2)
    m.conv1.bias = torch.nn.Parameter(torch.zeros(64))            # the pointer moves
    third = encoder.packed_stem(m.conv1)
    assert third[1] is not second[1] and float(third[1].abs().sum()) == 0
    with pytest.raises(RuntimeError, match="encoder_stem: conv1 must go from 3 to 64"):
        encoder.packed_stem(U.StemEncoder(in_channels=4).conv1)


def test_stem_refusal_accepts_the_reference_and_names_each_refusal(encoder):
    nn = torch.nn
    assert encoder.stem_refusal(U.StemEncoder()) is None
    assert encoder.stem_refusal(H.SmallEncoder()) is None and encoder.stem_refusal(T.TrunkEncoder()) is None

    def refused(why, **attrs):
        m = U.StemEncoder()
        for k, v in attrs.items():
            setattr(m, k, v)
        got = encoder.stem_refusal(m)
        assert isinstance(got, str) and why in got, (why, got)

    refused("conv1 must be a Conv2d, not Identity", conv1=nn.Identity())
    refused("conv1 must be a Conv2d", conv1=H.Returns(torch.zeros(1)))
    refused("conv1 must be 7 x 7 with stride 2", conv1=nn.Conv2d(3, 64, 3, stride=2, padding=1))
    refused("conv1 must be 7 x 7 with stride 2", conv1=nn.Conv2d(3, 64, 7, stride=1, padding=3))
    refused("conv1 must be 7 x 7 with stride 2", conv1=nn.Conv2d(3, 64, 7, stride=2, padding=2))
    refused("conv1 must be 7 x 7 with stride 2", conv1=nn.Conv2d(3, 64, 7, stride=2, padding=3, padding_mode="reflect"))
    refused("conv1 must be 7 x 7 with stride 2", conv1=nn.Conv2d(3, 64, 7, stride=2, padding=3, dilation=2))
    refused("conv1 must be 7 x 7 with stride 2", conv1=nn.Conv2d(3, 63, 7, stride=2, padding=3, groups=3))
    refused("conv1 must be 7 x 7 with stride 2", conv1=nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False))
    refused("conv1 must go from 3 to 64 channels, not 4 -> 64", conv1=nn.Conv2d(4, 64, 7, stride=2, padding=3))
    refused("conv1 must go from 3 to 64 channels, not 3 -> 32", conv1=nn.Conv2d(3, 32, 7, stride=2, padding=3))
    refused("norm1 must be an InstanceNorm2d (norm_fn \"instance\"), not BatchNorm2d", norm1=nn.BatchNorm2d(64))
    refused("norm1 must be an InstanceNorm2d (norm_fn \"instance\"), not Identity", norm1=nn.Identity())
    refused("without affine parameters", norm1=nn.InstanceNorm2d(64, affine=True))
    refused("running statistics", norm1=nn.InstanceNorm2d(64, track_running_stats=True))
    refused("norm1's eps must be 1e-5", norm1=nn.InstanceNorm2d(64, eps=1e-3))
    refused("relu1 must be an nn.ReLU, not LeakyReLU", relu1=nn.LeakyReLU(0.1))
    refused("relu1 must be an nn.ReLU, not Identity", relu1=nn.Identity())


class _Ran(Exception):
    pass


def _forward_reaches(encoder, monkeypatch, m, x, flag):
    """Runs `forward` up to layer1 (replaced by a layer that raises) and returns (the calls of encoder_stem, layer1's input)."""
    calls, seen = [], []

    def fake(x, conv1, out=None):
        calls.append((x, conv1))
        return torch.full((x.shape[0], 64, (x.shape[2] - 1) // 2 + 1, (x.shape[3] - 1) // 2 + 1), 7.0)

    class Stop(torch.nn.Module):
        def forward(self, x):
            seen.append(x)
            raise _Ran()

    monkeypatch.setattr(encoder, "encoder_stem", fake)
    monkeypatch.setattr(encoder, "DEVICE_STEM", flag)
    monkeypatch.setattr(encoder, "_gpu", lambda name, t, what: t)      # the path is chosen on the CPU here; nothing is launched
    m.layer1 = Stop()
    with pytest.raises(_Ran):
        encoder.forward(m, x)
    return calls, seen[0]


def test_forward_sends_a_real_stem_to_the_kernels_only_when_the_flag_is_on(encoder, monkeypatch):
    x = torch.rand(1, 3, 12, 20, generator=torch.Generator().manual_seed(5)) * 2 - 1
    m = H.SmallEncoder()
    calls, seen = _forward_reaches(encoder, monkeypatch, m, x, True)
    assert len(calls) == 1 and calls[0][0] is x and calls[0][1] is m.conv1
    assert seen.shape == (1, 64, 6, 10) and bool((seen == 7.0).all())
    m = H.SmallEncoder()
    calls, seen = _forward_reaches(encoder, monkeypatch, m, x, False)
    assert calls == [] and torch.equal(seen, m.relu1(m.norm1(m.conv1(x))))                     # exactly the three modules


def test_forward_leaves_any_other_stem_to_torch(encoder, monkeypatch):
    """An identity stem (the existing head test's stand-ins) and a 4-channel conv1 never reach the kernels and never raise."""
    x4 = torch.rand(1, 4, 12, 20, generator=torch.Generator().manual_seed(6))
    m = H.SmallEncoder()
    m.conv1 = torch.nn.Conv2d(4, 64, 7, stride=2, padding=3).requires_grad_(False)
    calls, seen = _forward_reaches(encoder, monkeypatch, m, x4, True)
    assert calls == [] and torch.equal(seen, m.relu1(m.norm1(m.conv1(x4))))
    m = H.SmallEncoder()
    m.conv1 = m.norm1 = m.relu1 = torch.nn.Identity()
    calls, seen = _forward_reaches(encoder, monkeypatch, m, x4, True)
    assert calls == [] and seen is x4
    m = H.SmallEncoder()
    m.norm1 = torch.nn.InstanceNorm2d(64, eps=1e-3)
    calls, __ = _forward_reaches(encoder, monkeypatch, m, x4[:, :3], True)
    assert calls == []
    assert isinstance(encoder.DEVICE_STEM, bool)


def test_cpu_tensors_raise(encoder):
    t = U.case_tensors("tiny")
    conv1 = U.conv1_of(t)
    with pytest.raises(RuntimeError, match="GPU"):
        encoder.encoder_stem(t["x"], conv1)
    ops = _lib.torch_ops(strict=True)
    w, b = encoder.packed_stem(conv1)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.encoder_stem(t["x"], w, b, torch.zeros(3, 64, 4, 3))


def test_symbols_are_exported_and_sources_listed():
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "batrack_encoder.h")).read()
    for name in ("bt_encoder_stem_workspace_bytes", "bt_encoder_stem"):
        assert hasattr(L, name) and name in header, name
    assert "#define BT_ENC_CIMG 3" in header and "#define BT_ENC_CSTEM 64" in header and "is not here" not in header
    assert "encoder_stem.hip" in _lib.SOURCES and "conv_tile.hpp" in _lib.HEADERS
    assert "encoder stem" in _lib.ERRORS[_lib.BT_EUNSUPPORTED]
    import batrack_amd.frontend
    from batrack_amd.frontend import encoder
    for name in ("pack_stem_weights", "packed_stem", "stem_refusal", "encoder_stem", "DEVICE_STEM"):
        assert hasattr(encoder, name), name
        assert f"encoder.{name}" in batrack_amd.frontend.__doc__, name
    ops = _lib.torch_ops(strict=True)
    assert str(ops.encoder_stem.default._schema) == "batrack_hip::encoder_stem(Tensor x, Tensor w, Tensor b, Tensor(a!) out) -> ()"
    assert "conv_stats.hip" in _lib.SOURCES                        # the statistics kernel, shared with the trunk
    src = open(os.path.join(_lib.CSRC, "encoder_stem.hip")).read() + open(os.path.join(_lib.CSRC, "conv_stats.hip")).read()
    assert "atomic" not in src                                     # no atomics of any kind
    assert "tile_store_stats<ST_NT, true" in src and "tile_order_stats(" in src and "tile_flush<ST_NT>" in src      # the shared tile, not a copy


def test_abi_refuses_before_any_hip_call():
    """Argument checks return their codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    EINVAL, EUNS = _lib.BT_EINVAL, _lib.BT_EUNSUPPORTED
    P, big = 256, 1 << 31                                          # never dereferenced: every call below is refused first

    def call(C=3, h=40, w=72, data=P, F=2, wp=P, bias=P, c_out=64, ws=P, out=P, x=True, view=None):
        v = dict(data=data, C=C, h=h, w=w, sf=C * h * w, sc=h * w, sy=w, sx=1)
        v.update(view or {})
        lx = _lib.EncoderLevel(*(v[n] for n in ("data", "C", "h", "w", "sf", "sc", "sy", "sx")))
        return L.bt_encoder_stem(ctypes.byref(lx) if x else None, wp, bias, c_out, F, ws, out, None)

    tiles = lambda h, w: ((h + 7) // 8) * ((w + 15) // 16)
    assert L.bt_encoder_stem_workspace_bytes(2, 40, 72) == 2 * tiles(20, 36) * 64 * 16 + 2 * 64 * 8
    assert L.bt_encoder_stem_workspace_bytes(1, 1, 1) == 64 * 16 + 64 * 8
    assert L.bt_encoder_stem_workspace_bytes(12, 384, 512) == 12 * 384 * 64 * 16 + 12 * 64 * 8       # 4.7 MB, no map
    for bad in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, -1), (big, 1, 1), (1, big, 1), (1, 1 << 14, 1 << 14), (8, 1 << 13, 1 << 12)):
        assert L.bt_encoder_stem_workspace_bytes(*bad) == 0, bad

    # ---- BT_EINVAL
    assert call(x=False) == EINVAL and call(data=None) == EINVAL
    for name in ("wp", "bias", "ws", "out"):
        assert call(**{name: None}) == EINVAL, name
    for k in (dict(F=0), dict(F=-1), dict(h=0), dict(w=0), dict(h=-3), dict(C=0), dict(C=-3), dict(c_out=0), dict(c_out=-64)):
        assert call(**k) == EINVAL, k
    for s in ("sf", "sc", "sy", "sx"):
        assert call(view={s: -1}) == EINVAL, s
    assert call(wp=264) == EINVAL and call(ws=264) == EINVAL        # read and written 16 bytes at a time

    # ---- BT_EUNSUPPORTED
    for k in (dict(C=4), dict(C=1), dict(C=64), dict(c_out=32), dict(c_out=128)):
        assert call(**k) == EUNS, k
    assert call(F=65536, h=1, w=1) == EUNS and call(F=big, h=1, w=1) == EUNS
    for k in (dict(h=big, w=1), dict(h=1, w=big), dict(h=1 << 15, w=1 << 15), dict(h=3, w=5, view=dict(sf=big)), dict(h=3, w=5, view=dict(sc=big)),
              dict(h=3, w=5, view=dict(sy=big)), dict(h=3, w=5, view=dict(sx=big)), dict(h=3, w=5, view=dict(sc=1 << 30)),
              dict(h=3, w=5, view=dict(sf=(1 << 31) - 1))):
        assert call(**k) == EUNS, k
    assert call(F=8, h=1 << 13, w=1 << 12, view=dict(sf=0, sc=0)) == EUNS      # 8 * 64 * 2^12 * 2^11 = 2^32 output elements, x within bounds
    assert call(F=2, h=1 << 13, w=1 << 13, view=dict(sf=0, sc=0)) == EUNS      # 2 * 64 * 2^24 = 2^31
