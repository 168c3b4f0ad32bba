"""CPU half of the encoder's head (include/batrack_encoder.h): the reference's fixture (tests/golden/encoder_head.npz, made by
its unmodified BasicEncoder.forward) against the torch restatement in tests/encoder_head_util.py; the input digests, the
weight repacks, the signature, install(), the refusals of `forward`, the ABI's refusals and the import surface — none of
which touch a GPU."""
import ctypes
import inspect
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import encoder_head_util as U
from batrack_amd import _lib

D = dict(np.load(U.GOLD))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated(c, dtype):
    t = U.case_tensors(c, dtype)
    with torch.no_grad():
        return U.head(*(t[n] for n in U.INPUTS), U.CASES[c]["size"])


@pytest.mark.parametrize("c", list(U.CASES))
def test_generator_reproduces_the_fixtures_inputs(c):
    d = U.make_inputs(**U.CASES[c])
    for name in U.INPUTS:
        assert np.array_equal(U.digest(d[name]), D[f"{c}.digest.{name}"]), name
        assert np.array_equal(d[name], d[name].astype(np.float32).astype(np.float64))
    for name in U.NAMES:
        assert d[name].min() >= 0                                 # maps after a ReLU
    assert float(np.abs(D[f"{c}.digest.b2"]).sum()) > 0 and float(np.abs(D[f"{c}.digest.b3"]).sum()) > 0


@pytest.mark.parametrize("c", list(U.CASES))
def test_float64_restatement_reproduces_the_float64_run(c):
    got = restated(c, torch.float64).numpy().ravel()[::U.F64_STEP]
    want = D[f"{c}.out64"]
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()


@pytest.mark.parametrize("c", list(U.CASES))
def test_float32_restatement_stays_within_the_gate(c):
    got, want, gate = restated(c, torch.float32).numpy(), D[f"{c}.out32"], float(D[f"{c}.gate"])
    assert got.shape == want.shape == (U.CASES[c]["F"], U.COUT, *U.CASES[c]["size"])
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"case {c}: max |restatement32 - ref32| {err:.3e}, gate {gate:.3e}")
    assert 0 < gate < 5e-5 and err <= gate


def test_fixture_cases_cover_what_they_claim():
    s4, s8, thin = (U.CASES[c] for c in ("s4", "s8", "thin"))
    assert s4["sizes"][1] == s4["size"] and s4["size"][0] % 8 and s4["size"][1] % 16 and s4["size"][1] > 16      # `b` identical; partial tiles; two across
    assert s8["sizes"][2] == s8["size"] and s8["sizes"][0][0] > s8["size"][0] < 2 * s8["sizes"][3][0]            # shrink, identical, grow
    assert thin["size"][0] == 1 and thin["sizes"][3] == (1, 1) and 32 < thin["size"][1] <= 48                   # one row, a 1 x 1 source, three tiles
    assert os.path.getsize(U.GOLD) < 600 * 1024


def test_resize_rule_of_the_header_is_torchs():
    """The header's align_corners rule, stated index by index in float32, against F.interpolate on the CPU.  Values below 1:
    either side rounds two products and a sum (torch may fuse them), 1.5 x 2^-24 from the exact blend each, so 3 x 2^-24
    between them; a wrong index or weight would be off by the difference of two neighbours."""
    g = torch.Generator().manual_seed(5)
    for (n_in, n_out) in ((18, 9), (37, 19), (5, 9), (3, 19), (1, 7), (4, 1), (9, 9)):
        src = torch.rand(1, 1, n_in, 1, generator=g)
        scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
        want = U.resize(src, (n_out, 1))[0, 0, :, 0]
        for o in range(n_out):
            s = np.float32(scale * np.float32(o))
            i0 = min(int(s), n_in - 1)
            i1 = min(i0 + 1, n_in - 1)
            l1 = np.float32(s - np.float32(i0))
            l0 = np.float32(np.float32(1) - l1)
            v = np.float32(np.float32(l0 * src[0, 0, i0, 0].numpy()) + np.float32(l1 * src[0, 0, i1, 0].numpy()))
            assert abs(float(v) - float(want[o])) <= 3 * 2.0 ** -24, (n_in, n_out, o)
    same = torch.rand(2, 3, 9, 19, generator=g)
    assert torch.equal(U.resize(same, (9, 19)), same)           # a level of the output's size is reproduced exactly


def test_repacks_are_permutations():
    from batrack_amd.frontend import encoder
    t = U.case_tensors("s8")
    p2, p3 = encoder.pack_head_weights(t["w2"], t["w3"])
    assert p2.shape == (52, 9, 8, 256) and p3.shape == (256, 128) and p2.is_contiguous() and p3.is_contiguous()
    w2, w3 = U.pack_head_weights(t["w2"], t["w3"])
    assert torch.equal(p2, w2) and torch.equal(p3, w3)
    assert p2[7, 5, 3, 200] == t["w2"][200, 59, 1, 2] and p2[8, 0, 0, 1] == t["w2"][1, 64, 0, 0] and p3[77, 5] == t["w3"][5, 77, 0, 0]
    assert torch.equal(torch.sort(p2.flatten())[0], torch.sort(t["w2"].flatten())[0])
    with pytest.raises(RuntimeError, match="416"):
        encoder.pack_head_weights(torch.zeros(256, 288, 3, 3), t["w3"])
    with pytest.raises(RuntimeError, match="1 x 1"):
        encoder.pack_head_weights(t["w2"], torch.zeros(128, 256, 3, 3))


def test_repack_is_cached_on_pointer_and_version():
    from batrack_amd.frontend import encoder
    conv2, conv3 = torch.nn.Conv2d(416, 256, 3, padding=1), torch.nn.Conv2d(256, 128, 1)
    a = encoder.packed_head(conv2, conv3)
    assert encoder.packed_head(conv2, conv3)[0] is a[0]
    with torch.no_grad():
        conv3.weight.mul_(2.0)
    b = encoder.packed_head(conv2, conv3)
    assert b[2] is not a[2] and torch.equal(b[2], encoder.pack_head_weights(conv2.weight, conv3.weight)[1])
    other = torch.nn.Conv2d(256, 128, 1)
    assert torch.equal(encoder.packed_head(conv2, other)[3], other.bias)
    for bad2, bad3, why in ((torch.nn.Conv2d(416, 256, 3, padding=0), conv3, "padding 1"),
                            (torch.nn.Conv2d(416, 256, 3, padding=1, padding_mode="reflect"), conv3, "zeros"),
                            (torch.nn.Conv2d(416, 256, 3, padding=1, stride=2), conv3, "stride 1"),
                            (torch.nn.Conv2d(416, 256, 3, padding=2, dilation=2), conv3, "dilation"),
                            (torch.nn.Conv2d(416, 256, 3, padding=1, groups=2), conv3, "one group"),
                            (torch.nn.Conv2d(416, 256, 3, padding=1, bias=False), conv3, "no bias"),
                            (conv2, torch.nn.Conv2d(256, 128, 1, stride=2), "stride 1"),
                            (conv2, torch.nn.Conv2d(256, 128, 3, padding=1), "1 x 1"),
                            (conv2, torch.nn.Conv2d(256, 128, 1, bias=False), "no bias")):
        with pytest.raises(RuntimeError, match=why):
            encoder.packed_head(bad2, bad3)


def test_signature_is_the_references():
    from batrack_amd.frontend import encoder
    got = str(inspect.signature(encoder.forward))
    assert got == str(D["signature"]) == "(self, x)"


def test_install_returns_the_previous_binding_and_is_idempotent():
    from batrack_amd.frontend import encoder
    mod = types.ModuleType("stand_in_blocks")
    old = lambda self, x: None
    mod.BasicEncoder = type("BasicEncoder", (), {"forward": old})
    assert encoder.install(mod) is old
    assert mod.BasicEncoder.forward is encoder.forward
    assert encoder.install(mod) is encoder.forward and mod.BasicEncoder.forward is encoder.forward


def test_forward_names_what_it_refuses():
    from batrack_amd.frontend import encoder
    x = torch.zeros(1, 3, 40, 72)
    m = U.SmallEncoder()
    m.shallow = True
    with pytest.raises(RuntimeError, match="shallow"):
        encoder.forward(m, x)
    for norm_fn in ("batch", "group", "none"):
        with pytest.raises(RuntimeError, match="norm_fn"):
            encoder.forward(U.SmallEncoder(norm_fn=norm_fn), x)
    m = U.SmallEncoder()
    m.norm2 = torch.nn.InstanceNorm2d(256, affine=True)
    with pytest.raises(RuntimeError, match="affine"):
        encoder.forward(m, x)
    m.norm2 = torch.nn.InstanceNorm2d(256, track_running_stats=True)
    with pytest.raises(RuntimeError, match="running statistics"):
        encoder.forward(m, x)
    m.norm2 = torch.nn.BatchNorm2d(256)
    with pytest.raises(RuntimeError, match="InstanceNorm2d"):
        encoder.forward(m, x)
    m = U.SmallEncoder(dropout=0.1)
    m.train()
    with pytest.raises(RuntimeError, match="dropout"):
        encoder.forward(m, x)
    with pytest.raises(RuntimeError, match="GPU"):                # eval with dropout, and every other check, passes: the CPU tensor does not
        encoder.forward(m.eval(), x)
    with pytest.raises(RuntimeError, match="GPU"):
        encoder.forward(U.SmallEncoder(), x)


def test_cpu_tensors_raise():
    from batrack_amd.frontend import encoder
    t = U.case_tensors("s8")
    conv2, conv3 = U.convs(t)
    with pytest.raises(RuntimeError, match="GPU"):
        encoder.encoder_head(*(t[n] for n in U.NAMES), conv2, conv3, U.CASES["s8"]["size"])
    ops = _lib.torch_ops(strict=True)
    p2, p3 = encoder.pack_head_weights(t["w2"], t["w3"])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.encoder_head(*(t[n] for n in U.NAMES), p2, t["b2"], p3, t["b3"], torch.zeros(1, 128, 5, 17))


def test_symbols_are_exported_and_sources_listed():
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "batrack_encoder.h")).read()
    for name in ("bt_encoder_head_workspace_bytes", "bt_encoder_head"):
        assert hasattr(L, name) and name in header, name
    assert "encoder_head.hip" in _lib.SOURCES and any(h.endswith("batrack_encoder.h") for h in _lib.HEADERS)
    assert "encoder head" in _lib.ERRORS[_lib.BT_EUNSUPPORTED]
    import batrack_amd.frontend
    assert "encoder.forward" in batrack_amd.frontend.__doc__
    ops = _lib.torch_ops(strict=True)
    assert str(ops.encoder_head.default._schema) == (
        "batrack_hip::encoder_head(Tensor a, Tensor b, Tensor c, Tensor d, Tensor w2_packed, Tensor bias2, Tensor w3_packed, Tensor bias3, "
        "Tensor(a!) out) -> ()")


def test_abi_refuses_before_any_hip_call():
    """Argument checks return their codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    EINVAL, EUNS = _lib.BT_EINVAL, _lib.BT_EUNSUPPORTED
    p, big = ctypes.c_void_p(256), 1 << 31                    # never dereferenced: every call below is refused first
    F, h, w = 2, 9, 19

    def level(C, hl, wl, data=256, **k):
        v = dict(data=data, C=C, h=hl, w=wl, sf=C * hl * wl, sc=hl * wl, sy=wl, sx=1)
        v.update(k)
        return _lib.EncoderLevel(*(v[n] for n in ("data", "C", "h", "w", "sf", "sc", "sy", "sx")))

    good = dict(a=level(64, 18, 37), b=level(96, 9, 19), c=level(128, 5, 10), d=level(128, 3, 5), w2=p, b2=p, cmid=256, w3=p, b3=p,
                cout=128, F=F, h=h, w=w, ws=p, out=p)

    def call(**k):
        v = dict(good, **k)
        lv = [ctypes.byref(v[n]) if v[n] is not None else None for n in "abcd"]
        return L.bt_encoder_head(*lv, *(v[n] for n in ("w2", "b2", "cmid", "w3", "b3", "cout", "F", "h", "w", "ws", "out")), None)

    assert L.bt_encoder_head_workspace_bytes(F, h, w) == F * 256 * h * w * 4 + F * 2 * 2 * 256 * 16
    assert L.bt_encoder_head_workspace_bytes(1, 1, 1) == 1024 + 256 * 16
    for bad in ((0, 9, 19), (2, 0, 19), (2, 9, -1), (1, 1 << 12, 1 << 11), (big, 1, 1)):
        assert L.bt_encoder_head_workspace_bytes(*bad) == 0, bad

    for name in ("a", "b", "c", "d", "w2", "b2", "w3", "b3", "ws", "out"):
        assert call(**{name: None}) == EINVAL, name
    for name in "abcd":
        assert call(**{name: level(good[name].C, 3, 5, data=None)}) == EINVAL, name
        for k in (dict(hl=0, wl=5), dict(hl=3, wl=0), dict(hl=-1, wl=5)):
            assert call(**{name: level(good[name].C, **k)}) == EINVAL, (name, k)
        for k in (dict(sf=-1), dict(sc=-1), dict(sy=-1), dict(sx=-1)):
            assert call(**{name: level(good[name].C, 3, 5, **k)}) == EINVAL, (name, k)
    for k in (dict(F=0), dict(h=0), dict(w=0), dict(F=-1), dict(cmid=0), dict(cout=-1)):
        assert call(**k) == EINVAL, k
    for name in ("w2", "w3", "ws"):                             # read and written 16 bytes at a time
        assert call(**{name: ctypes.c_void_p(264)}) == EINVAL, name

    for name, C in (("a", 96), ("a", 63), ("b", 64), ("c", 96), ("d", 64), ("d", 129)):
        assert call(**{name: level(C, 3, 5)}) == EUNS, (name, C)
    for k in (dict(cmid=128), dict(cmid=257), dict(cout=256), dict(cout=64)):
        assert call(**k) == EUNS, k
    for k in (dict(F=big), dict(h=big), dict(w=big), dict(F=1, h=1 << 12, w=1 << 11), dict(F=65536, h=1, w=1)):
        assert call(**k) == EUNS, k
    for name in "abcd":
        C = good[name].C
        for k in (dict(hl=big, wl=1), dict(hl=1, wl=big), dict(hl=1 << 13, wl=1 << 12), dict(hl=3, wl=5, sf=big), dict(hl=3, wl=5, sc=big),
                  dict(hl=3, wl=5, sy=big), dict(hl=3, wl=5, sx=big), dict(hl=3, wl=5, sc=1 << 26),dict(hl=3, wl=5, sf=(1 << 31) - 1)):
            assert call(**{name: level(C, **k)}) == EUNS, (name, k)


def test_import_surface():
    """Importing the module loads no native library, no oracle and no test module."""
    code = ("import sys; import batrack_amd.frontend.encoder; from batrack_amd import _lib; "
            "assert 'oracle' not in sys.modules and 'tests' not in sys.modules and 'encoder_head_util' not in sys.modules; "
            "assert _lib._lib is None and _lib._torch_ops is None; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
    for name in ("encoder.py",):
        src = open(os.path.join(ROOT, "batrack_amd", "frontend", name)).read()
        assert "import oracle" not in src and "import tests" not in src and "from tests" not in src and "from oracle" not in src
