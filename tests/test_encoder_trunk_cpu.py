"""CPU half of the encoder's trunk (bt_res_block in include/batrack_encoder.h): the reference's fixture
(tests/golden/encoder_trunk.npz, made by its unmodified residual blocks) against the torch restatement in
tests/encoder_trunk_util.py; the input digests, the weight repacks and their cache, the block recogniser and its refusals,
the ABI's refusals and the import surface — none of which touch a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import encoder_head_util as H
import encoder_trunk_util as U
from batrack_amd import _lib

D = dict(np.load(U.GOLD))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def restated():
    """Per case and dtype: (the four levels of the whole run, the four layers each alone on its own input)."""
    runs = {}
    for c in U.CASES:
        for dtype in (torch.float32, torch.float64):
            t = U.case_tensors(c, dtype)
            with torch.no_grad():
                runs[c, dtype] = (U.trunk(t["x"], t), [U.layer(U.layer_input(t, name), t, name) for name in U.LAYERS])
    return runs


@pytest.mark.parametrize("c", list(U.CASES))
def test_generator_reproduces_the_fixtures_inputs(c):
    d = U.make_inputs(**U.CASES[c])
    assert set(d) == {"x", "in.layer2", "in.layer3", "in.layer4"} | set(U.weight_names())
    for name, v in d.items():
        assert np.array_equal(U.digest(v), D[f"{c}.digest.{name}"]), name
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
        if name.endswith("bias"):
            assert np.abs(v).max() <= 0.5 and np.abs(v).sum() > 0          # uniform in +-0.5, not zero
    for name in ("x", "in.layer2", "in.layer3", "in.layer4"):
        assert d[name].min() >= 0                                  # maps after a ReLU


@pytest.mark.parametrize("c", list(U.CASES))
def test_float64_restatement_reproduces_the_float64_runs(c, restated):
    whole, alone = restated[c, torch.float64]
    for i, l in enumerate(U.LEVELS):
        for got, key in ((whole[i], "out64"), (alone[i], "layer64")):
            got, want = got.numpy().ravel()[::U.STEP[l]], D[f"{c}.{l}.{key}"]
            assert got.shape == want.shape and want.dtype == np.float64
            assert np.abs(got - want).max() <= 1e-12, (l, key, np.abs(got - want).max())


@pytest.mark.parametrize("c", list(U.CASES))
def test_float32_restatement_stays_within_the_gates(c, restated):
    whole, alone = restated[c, torch.float32]
    for i, l in enumerate(U.LEVELS):
        s, gate, lgate = U.STEP[l], float(D[f"{c}.{l}.gate"]), float(D[f"{c}.{l}.layer_gate"])
        assert tuple(whole[i].shape) == (U.CASES[c]["F"], U.BLOCKS[2 * i][3], *U.level_sizes(U.CASES[c]["size"])[i])
        err = float(np.abs(whole[i].numpy().ravel()[::s].astype(np.float64) - D[f"{c}.{l}.out32"]).max())
        err64 = float(np.abs(alone[i].numpy().ravel()[::s].astype(np.float64) - D[f"{c}.{l}.layer64"]).max())
        print(f"case {c} level {l}: max |restatement32 - ref32| {err:.3e}, gate {gate:.3e}; alone against float64 {err64:.3e}, gate {lgate:.3e}")
        assert 0 < gate < 5e-5 and 0 < lgate < 5e-5 and err <= gate        # (a layer alone has no stored float32 run: printed only)


def test_fixture_cases_cover_what_they_claim():
    even, odd, exact = (U.level_sizes(U.CASES[c]["size"]) for c in ("even", "odd", "exact"))
    assert even == ((20, 36), (10, 18), (5, 9), (3, 5)) and odd == ((17, 33), (9, 17), (5, 9), (3, 5)) and exact == ((24, 32), (12, 16), (6, 8), (3, 4))
    assert U.CASES["even"]["F"] == 2 and even[0][0] > 16 and even[0][1] > 32                # several tiles both ways
    assert exact[0][0] % 8 == 0 and exact[0][1] % 16 == 0 and exact[1][1] % 16 == 0              # exact tiles
    for sizes in (even, odd, exact):
        assert sizes[3][0] * sizes[3][1] >= 12                                                # the 12-pixel condition
        for l, (h, w) in zip(U.LEVELS, sizes):
            assert np.gcd(U.STEP[l], w) == 1                                                  # the samples sweep the columns
    assert os.path.getsize(U.GOLD) <= os.path.getsize(H.GOLD)


def test_conditions_reject_what_they_should():
    g = torch.Generator().manual_seed(3)
    ok = torch.randn(1, 4, 3, 4, generator=g)
    assert U.conditions_hold([ok]) and not U.conditions_hold([ok[:, :, :1, :2]])
    flat = ok.clone()
    flat[0, 2] = 0.25
    assert not U.conditions_hold([flat])


def test_repacks_are_permutations():
    from batrack_amd.frontend import encoder
    t = U.case_tensors("odd")
    for layer, i, c_in, c_out, stride in U.BLOCKS:
        w1, __, w2, __, wd, __ = U.block_args(t, layer, i)
        p1, p2, pd = encoder.pack_block_weights(w1, w2, wd)
        q1, q2, qd = U.pack_block_weights(w1, w2, wd)
        assert p1.shape == (c_in // 8, 9, 8, c_out) and p2.shape == (c_out // 8, 9, 8, c_out) and p1.is_contiguous() and p2.is_contiguous()
        assert torch.equal(p1, q1) and torch.equal(p2, q2)
        assert p1[c_in // 8 - 1, 5, 3, c_out - 2] == w1[c_out - 2, c_in - 5, 1, 2] and p2[1, 0, 0, 1] == w2[1, 8, 0, 0]
        assert torch.equal(torch.sort(p1.flatten())[0], torch.sort(w1.flatten())[0])
        if stride == 2:
            assert pd.shape == (c_in, c_out) and pd.is_contiguous() and torch.equal(pd, qd) and pd[7, 5] == wd[5, 7, 0, 0]
        else:
            assert pd is None and wd is None
    with pytest.raises(RuntimeError, match="64, 96 or 128"):
        encoder.pack_block_weights(torch.zeros(64, 32, 3, 3), torch.zeros(64, 64, 3, 3))
    with pytest.raises(RuntimeError, match="conv2"):
        encoder.pack_block_weights(torch.zeros(96, 64, 3, 3), torch.zeros(96, 64, 3, 3))
    with pytest.raises(RuntimeError, match="downsample"):
        encoder.pack_block_weights(torch.zeros(96, 64, 3, 3), torch.zeros(96, 96, 3, 3), torch.zeros(96, 96, 1, 1))


def test_repack_is_cached_on_pointer_and_version():
    from batrack_amd.frontend import encoder
    b = U.Block(64, 96, 2)
    first = encoder.packed_block(b)
    assert all(x is y for x, y in zip(encoder.packed_block(b), first))
    assert len(first) == 6 and torch.equal(first[5], b.downsample[0].bias)
    with torch.no_grad():
        b.downsample[0].weight.mul_(2.0)                          # the version moves
    second = encoder.packed_block(b)
    assert second[4] is not first[4] and torch.equal(second[4], encoder.pack_block_weights(b.conv1.weight, b.conv2.weight, b.downsample[0].weight)[2])
    b.conv2.weight = torch.nn.Parameter(torch.zeros_like(b.conv2.weight))     # the pointer moves
    third = encoder.packed_block(b)
    assert third[2] is not second[2] and float(third[2].abs().sum()) == 0
    plain = encoder.packed_block(U.Block(128, 128, 1))
    assert plain[4] is None and plain[5] is None


def test_recogniser_accepts_the_shape_and_names_each_refusal():
    from batrack_amd.frontend import encoder
    for __, __, c_in, c_out, stride in U.BLOCKS:
        assert encoder.check_block(U.Block(c_in, c_out, stride)) == stride
    assert all(encoder.is_residual_layer(l) for l in U.make_layers())

    def refused(why, edit, c_in=64, c_out=96, stride=2):
        b = U.Block(c_in, c_out, stride)
        edit(b)
        assert encoder.is_residual_shaped(b)                     # residual-shaped: refused loudly, not left to torch
        with pytest.raises(RuntimeError, match=why):
            encoder.packed_block(b)

    nn = torch.nn
    refused("norm1 must be an InstanceNorm2d", lambda b: setattr(b, "norm1", nn.BatchNorm2d(96)))
    refused("norm2 must be an InstanceNorm2d", lambda b: setattr(b, "norm2", nn.GroupNorm(12, 96)))
    refused("norm1 .* affine", lambda b: setattr(b, "norm1", nn.InstanceNorm2d(96, affine=True)))
    refused("norm2 .* running statistics", lambda b: setattr(b, "norm2", nn.InstanceNorm2d(96, track_running_stats=True)))
    refused("norm1's eps", lambda b: setattr(b, "norm1", nn.InstanceNorm2d(96, eps=1e-3)))
    refused(r"downsample\[1\]", lambda b: b.downsample.__setitem__(1, nn.BatchNorm2d(96)))
    refused(r"downsample\[1\]'s eps", lambda b: b.downsample.__setitem__(1, nn.InstanceNorm2d(96, eps=1e-6)))
    refused("conv1 must be 3 x 3 with padding 1", lambda b: setattr(b, "conv1", nn.Conv2d(64, 96, 3, stride=2, padding=1, padding_mode="reflect")))
    refused("conv1 must be 3 x 3 with padding 1", lambda b: setattr(b, "conv1", nn.Conv2d(64, 96, 3, stride=2, padding=1, bias=False)))
    refused("conv1 must be 3 x 3 with padding 1", lambda b: setattr(b, "conv1", nn.Conv2d(64, 96, 3, stride=3, padding=1)))
    refused("conv2 must be 3 x 3 with padding 1 .* stride 1", lambda b: setattr(b, "conv2", nn.Conv2d(96, 96, 3, stride=2, padding=1)))
    refused("channel counts must be 64, 96 or 128", lambda b: setattr(b, "conv1", nn.Conv2d(32, 96, 3, stride=2, padding=1)))
    refused("channel counts must be 64, 96 or 128", lambda b: setattr(b, "conv2", nn.Conv2d(96, 128, 3, padding=1)))
    refused("stride-2 block's downsample", lambda b: setattr(b, "downsample", None))
    refused("stride-2 block's downsample", lambda b: setattr(b, "downsample", nn.Sequential(b.downsample[0])))
    refused(r"downsample\[0\] must be 1 x 1 with stride 2", lambda b: b.downsample.__setitem__(0, nn.Conv2d(64, 96, 1, stride=1)))
    refused(r"downsample\[0\] must be 1 x 1 with stride 2", lambda b: b.downsample.__setitem__(0, nn.Conv2d(64, 96, 1, stride=2, padding=1)))
    refused("stride-1 block must have downsample None", lambda b: setattr(b, "downsample", nn.Sequential(nn.Conv2d(64, 64, 1), nn.InstanceNorm2d(64))),
            64, 64, 1)
    refused("stride-1 block must keep its channel count", lambda b: (setattr(b, "conv1", nn.Conv2d(64, 96, 3, padding=1)),
                                                                      setattr(b, "conv2", nn.Conv2d(96, 96, 3, padding=1))), 64, 64, 1)


def test_a_layer_that_is_not_residual_is_left_to_itself():
    from batrack_amd.frontend import encoder
    m = H.SmallEncoder()
    for layer in (m.layer1, m.layer4, H.Returns(torch.zeros(1)), torch.nn.Sequential(), torch.nn.Identity(),
                  torch.nn.Sequential(U.Block(64, 64), torch.nn.ReLU())):
        assert not encoder.is_residual_layer(layer)
    assert set(encoder.DEVICE_LAYERS) <= set(U.LAYERS)
    with pytest.raises(RuntimeError, match="layer1 must be a Sequential of residual blocks"):
        encoder.encoder_trunk(torch.zeros(1, 64, 4, 4), m.layer1, m.layer2, m.layer3, m.layer4)
    src = open(os.path.join(ROOT, "batrack_amd", "frontend", "encoder.py")).read()
    assert "if name in DEVICE_LAYERS and is_residual_layer(layer) else layer(x)" in src      # `forward` calls any other layer as it is


def test_cpu_tensors_raise():
    from batrack_amd.frontend import encoder
    t = U.case_tensors("odd")
    layers = U.make_layers(t)
    with pytest.raises(RuntimeError, match="GPU"):
        encoder.residual_block(t["x"], layers[0][0])
    with pytest.raises(RuntimeError, match="GPU"):
        encoder.encoder_trunk(t["x"], *layers)
    with pytest.raises(RuntimeError, match="GPU"):
        encoder.forward(U.TrunkEncoder(), torch.zeros(1, 3, 40, 72))
    ops = _lib.torch_ops(strict=True)
    w1, b1, w2, b2, wd, bd = encoder.packed_block(layers[0][0])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.res_block(t["x"], w1, b1, w2, b2, wd, bd, 1, torch.zeros(1, 64, 17, 33))


def test_symbols_are_exported_and_sources_listed():
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "batrack_encoder.h")).read()
    for name in ("bt_res_block_workspace_bytes", "bt_res_block"):
        assert hasattr(L, name) and name in header, name
    assert "encoder_trunk.hip" in _lib.SOURCES and "conv_tile.hpp" in _lib.HEADERS
    assert "residual block" in _lib.ERRORS[_lib.BT_EUNSUPPORTED]
    assert [n for n, __ in _lib.ResBlock._fields_] == ["w1", "b1", "w2", "b2", "wd", "bd", "c_in", "c_out", "stride"]
    import batrack_amd.frontend
    from batrack_amd.frontend import encoder
    for name in ("pack_block_weights", "packed_block", "residual_block", "encoder_trunk", "DEVICE_LAYERS"):
        assert hasattr(encoder, name), name
        assert name == "DEVICE_LAYERS" or f"encoder.{name}" in batrack_amd.frontend.__doc__, name
    ops = _lib.torch_ops(strict=True)
    assert str(ops.res_block.default._schema) == ("batrack_hip::res_block(Tensor x, Tensor w1, Tensor b1, Tensor w2, Tensor b2, Tensor? wd, "
                                                  "Tensor? bd, int stride, Tensor(a!) out) -> ()")
    src = open(os.path.join(_lib.CSRC, "encoder_trunk.hip")).read() + open(os.path.join(_lib.CSRC, "conv_tile.hpp")).read()
    assert "atomic" not in src.replace("No atomics", "").replace("no floating-point atomics", "")      # no atomics of any kind


def test_abi_refuses_before_any_hip_call():
    """Argument checks return their codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    EINVAL, EUNS = _lib.BT_EINVAL, _lib.BT_EUNSUPPORTED
    P, big = 256, 1 << 31                                          # never dereferenced: every call below is refused first

    def call(C=64, h=20, w=36, data=P, F=2, ws=P, out=P, x=True, blk=True, view=None, **k):
        v = dict(data=data, C=C, h=h, w=w, sf=C * h * w, sc=h * w, sy=w, sx=1)
        v.update(view or {})
        lx = _lib.EncoderLevel(*(v[n] for n in ("data", "C", "h", "w", "sf", "sc", "sy", "sx")))
        b = dict(w1=P, b1=P, w2=P, b2=P, wd=P, bd=P, c_in=64, c_out=96, stride=2)
        b.update(k)
        rb = _lib.ResBlock(*(b[n] for n in ("w1", "b1", "w2", "b2", "wd", "bd", "c_in", "c_out", "stride")))
        return L.bt_res_block(ctypes.byref(lx) if x else None, ctypes.byref(rb) if blk else None, F, ws, out, None)

    s1 = dict(c_in=64, c_out=64, stride=1, wd=None, bd=None)
    tiles = lambda h, w: ((h + 7) // 8) * ((w + 15) // 16)
    assert L.bt_res_block_workspace_bytes(2, 96, 20, 36, 2) == 3 * 2 * 96 * 180 * 4 + 3 * 2 * tiles(10, 18) * 96 * 16 + 3 * 2 * 96 * 8
    assert L.bt_res_block_workspace_bytes(1, 64, 1, 1, 1) == 2 * 64 * 4 + 2 * 64 * 16 + 2 * 64 * 8
    assert L.bt_res_block_workspace_bytes(1, 128, 17, 33, 2) == ((3 * 128 * 153 * 4 + 15) // 16) * 16 + 3 * tiles(9, 17) * 128 * 16 + 3 * 128 * 8
    for bad in ((0, 64, 4, 4, 1), (1, 64, 0, 4, 1), (1, 64, 4, -1, 1), (1, 32, 4, 4, 1), (1, 64, 4, 4, 0), (1, 64, 4, 4, 3), (big, 64, 1, 1, 1),
                (1, 128, 1 << 12, 1 << 11, 1), (2, 128, 1 << 12, 1 << 12, 2)):
        assert L.bt_res_block_workspace_bytes(*bad) == 0, bad

    # ---- BT_EINVAL
    assert call(x=False) == EINVAL and call(blk=False) == EINVAL and call(data=None) == EINVAL
    for name in ("ws", "out"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("w1", "b1", "w2", "b2"):
        assert call(**{name: None}) == EINVAL, name
    for k in (dict(F=0), dict(F=-1), dict(h=0), dict(w=0), dict(h=-3), dict(C=0), dict(c_in=0), dict(c_out=-64), dict(stride=0), dict(stride=-1)):
        assert call(**k) == EINVAL, k
    for s in ("sf", "sc", "sy", "sx"):
        assert call(view={s: -1}) == EINVAL, s
    for name in ("w1", "w2", "wd"):                               # read 16 bytes at a time
        assert call(**{name: 264}) == EINVAL, name
    assert call(ws=264) == EINVAL
    assert call(wd=None) == EINVAL and call(bd=None) == EINVAL and call(wd=None, bd=None) == EINVAL      # absent at stride 2
    assert call(**dict(s1, wd=P, bd=P)) == EINVAL and call(**dict(s1, wd=P)) == EINVAL and call(**dict(s1, bd=P)) == EINVAL

    # ---- BT_EUNSUPPORTED
    for k in (dict(C=32, c_in=32), dict(C=72, c_in=72), dict(C=256, c_in=256), dict(c_out=32), dict(c_out=112), dict(c_out=256)):
        assert call(**k) == EUNS, k
    assert call(C=96) == EUNS                                       # the view's channels are not the block's
    assert call(stride=3) == EUNS and call(stride=4, wd=None, bd=None) == EUNS
    assert call(**dict(s1, c_out=96)) == EUNS and call(**dict(s1, c_in=96, C=96)) == EUNS      # stride 1 keeps its channels
    assert call(F=65536, h=1, w=1) == EUNS and call(F=big, h=1, w=1) == EUNS
    for k in (dict(h=big, w=1), dict(h=1, w=big), dict(h=1 << 13, w=1 << 12), dict(h=3, w=5, view=dict(sf=big)), dict(h=3, w=5, view=dict(sc=big)),
              dict(h=3, w=5, view=dict(sy=big)), dict(h=3, w=5, view=dict(sx=big)), dict(h=3, w=5, view=dict(sc=1 << 26)),
              dict(h=3, w=5, view=dict(sf=(1 << 31) - 1))):
        assert call(**k) == EUNS, k
    assert call(F=1, h=1 << 12, w=(1 << 12) + 64, **dict(s1, c_in=128, c_out=128), C=128, view=dict(sf=0, sc=0)) == EUNS      # x's element count
    assert call(F=8, h=1 << 11, w=1 << 10, **s1, view=dict(sf=0, sc=0)) == EUNS           # 2 maps * 8 * 64 * 2^21 = 2^31 in the workspace
