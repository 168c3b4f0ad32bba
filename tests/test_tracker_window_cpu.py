"""CPU half of the tracker's window loop (include/batrack_window.h): the reference's fixture (tests/golden/tracker_window.npz,
made by its unmodified MDTracker.forward) against the torch restatement in tests/tracker_window_util.py; the input digests,
the weight repack, the signature, install(), the ABI's refusals and the import surface — none of which touch a GPU."""
import ctypes
import inspect
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import tracker_window_util as U
from batrack_amd import _lib

D = dict(np.load(U.GOLD))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated(c, dtype):
    me = U.StandIn(c, dtype, "cpu", U.embed3d_stand_in())
    T = U.case_tensors(c, dtype)
    with torch.no_grad():
        ret = U.forward(me, T["rgbds"], T["queries"])
    return me, T, ret


def windows_of(me):
    """The recorded calls with `fmaps` cut to the frames the window computed, as the fixture stores them."""
    S, first, out, ind, call = me.S, me.spec["first"], [], 0, 0
    for k, seen in enumerate(me.seen):
        while not any(f < ind + S for f in first):            # windows without a query call the encoder and nothing else
            ind, call = ind + S // 2, call + 1
        out.append(dict(seen, fmaps=seen["fmaps"][0, U.computed_frames(call, S)]))
        ind, call = ind + S // 2, call + 1
    return out


@pytest.fixture(scope="module", params=list(U.CASES))
def case(request):
    c = request.param
    return c, restated(c, torch.float32), restated(c, torch.float64)


def test_generator_reproduces_the_fixtures_inputs(case):
    c = case[0]
    d = U.make_inputs(**U.CASES[c])
    for name in U.INPUTS:
        assert np.array_equal(U.digest(d[name]), D[f"{c}.digest.{name}"]), name
        assert np.array_equal(d[name], d[name].astype(np.float32).astype(np.float64))


def test_float64_restatement_reproduces_the_float64_run(case):
    c, _, (me, T, ret) = case
    wins = windows_of(me)
    assert len(wins) == sum(1 for k in D if k.startswith(f"{c}.") and k.endswith(".f64.dmaps"))
    for k, win in enumerate(wins):
        for name in U.WINDOW_KEYS[:-1] + ("fmaps",):
            want = D[f"{c}.{k}.f64.{name}"]
            got = win[name].double().numpy()
            got = got.ravel()[::U.F64_STEP] if name == "fmaps" else got
            assert got.shape == want.shape, (c, k, name)
            assert np.abs(got - want).max() <= 1e-12, (c, k, name, np.abs(got - want).max())
        assert np.array_equal(win["track_mask"].numpy(), D[f"{c}.{k}.track_mask"])
    for name, got in zip(U.RETURNS, ret):
        assert np.abs(got.double().numpy() - D[f"{c}.f64.{name}"]).max() <= 1e-12, (c, name)
    assert (me.d_near, me.d_far) == tuple(D[f"{c}.d_range"])


def test_float32_restatement_stays_within_the_gate(case):
    """The copies, the masks and the depth maps bit for bit; everything else within the reference's own float32-vs-float64
    difference."""
    c, (me, T, ret), _ = case
    for k, win in enumerate(windows_of(me)):
        for name in U.WINDOW_KEYS + ("fmaps",):
            want, got = D[f"{c}.{k}.{name}"], win[name].numpy()
            if name in ("track_mask", "vis_init", "dmaps", "coords_init", "coords_dyn_init"):
                assert np.array_equal(got, want), (c, k, name)
                continue
            gate = float(D[f"gate.{c}.{name}"])
            err = float(np.abs(got.astype(np.float64) - want).max())
            print(f"case {c} window {k} {name}: max |restatement - ref32| {err:.3e}, gate {gate:.3e}")
            assert 0 < gate < 5e-4 and err <= gate, (c, k, name, err, gate)
    for name, got in zip(U.RETURNS, ret):
        want = D[f"{c}.{name}"]
        if name in ("traj_e", "depth_e", "traj_static_e"):
            assert np.array_equal(got.numpy(), want), (c, name)
        else:
            assert np.abs(got.numpy().astype(np.float64) - want).max() <= max(float(D[f"gate.{c}.{name}"]), 2.4e-7), (c, name)
    assert np.array_equal(U.digest(T["rgbds"].numpy()), D[f"{c}.rgbds_digest"])          # normalised in place, as the reference does


def test_fixture_cases_cover_what_they_claim():
    A, B, Cc = (U.CASES[c] for c in "ABC")
    assert (A["S"], A["T"], A["H"] // 4, A["W"] // 4, A["first"]) == (4, 7, 5, 7, (0, 0, 1, 3, 4, 5, 2))
    assert (B["S"], B["T"], B["H"] // 4, B["W"] // 4, len(B["first"])) == (2, 3, 9, 18, 3)
    assert (Cc["S"], Cc["T"], Cc["H"] // 4, Cc["W"] // 4, len(Cc["first"])) == (4, 4, 5, 7, 2)
    n = [D[f"A.{k}.coords_init"].shape[2] for k in range(3)]
    assert n == [5, 7, 7]                                        # tracks join in the first two windows, none in the last
    assert D["A.0.fmaps"].shape[0] == 4 and D["A.1.fmaps"].shape[0] == 2 and D["A.2.fmaps"].shape[0] == 2     # two sliding halves
    assert np.array_equal(D["A.2.dmaps"][0, 3], D["A.2.dmaps"][0, 2])                    # the padded last window
    assert "C.1.dmaps" not in D                                  # the single-window call
    for c, spec in U.CASES.items():
        q = U.make_inputs(**spec)["queries"][0]
        assert q[:, 1].min() < -2 and q[:, 1].max() > spec["W"] + 2 and q[:, 2].min() < -2 and q[:, 2].max() > spec["H"] + 2
        assert float(np.abs(D[f"{c}.digest.conv_b"]).sum()) > 0
    assert os.path.getsize(U.GOLD) < 600 * 1024


def test_repack_is_a_permutation():
    from batrack_amd.frontend import tracker
    w = torch.as_tensor(U.make_inputs(**U.CASES["C"])["conv_w"], dtype=torch.float32)
    got = tracker.pack_weights(w)
    assert got.shape == (24, 9, 8, 128) and got.is_contiguous()
    assert torch.equal(got, U.pack_weights(w))
    assert torch.equal(got.reshape(24, 9, 8, 128)[23, :, 7], torch.zeros(9, 128))        # the padding channel
    assert torch.equal(torch.sort(got.flatten()[got.flatten() != 0])[0], torch.sort(w.flatten()[w.flatten() != 0])[0])
    with pytest.raises(RuntimeError, match="191"):
        tracker.pack_weights(torch.zeros(128, 128, 3, 3))


def test_one_hot_convolutions_cover_every_pair_and_select_what_the_convolution_does():
    """The limits suite's one-hot convolutions: every (input channel, tap) pair has a weight of 1 in some convolution, and
    the expectation built by padding and slicing is what the restated convolution computes with those weights in float64."""
    taps = U.one_hot_taps()
    assert taps.shape == (U.ONE_HOT_CONVS, U.C, 3)
    flat = (taps[..., 0] * 9 + taps[..., 1] * 3 + taps[..., 2]).flatten()
    count = torch.bincount(flat, minlength=(U.C + U.EMB) * 9)
    assert count.numel() == 1719 and int(count.min()) >= 1 and int((count - 1).sum()) == 73
    assert int(taps[..., 0].max()) == 190 and int(taps[..., 1:].max()) == 2 and int(taps.min()) == 0
    S, frame0, F, h, w = 3, 1, 2, 9, 17
    g = torch.Generator().manual_seed(84)
    fnet = torch.randn(F, U.C, h, w, generator=g, dtype=torch.float64)
    dm = torch.rand(S, h, w, generator=g, dtype=torch.float64) * 17
    zr = (dm.min(), dm.max())
    inp = torch.cat([fnet, U.embedding(dm, zr)[frame0:frame0 + F]], 1)
    worst = 0.0
    for k in range(U.ONE_HOT_CONVS):
        weight, bias = U.one_hot_weight(taps[k], torch.float64), torch.rand(U.C, generator=g, dtype=torch.float64) - 0.5
        assert int((weight != 0).sum()) == U.C and float(weight.sum()) == U.C
        want = U.one_hot_select(inp, taps[k]) + bias[None, :, None, None]
        got = U.embed_conv(fnet, dm, zr, frame0, weight, bias)
        worst = max(worst, float((got - want).abs().max()))
        assert torch.equal(U.pack_weights(weight).permute(3, 0, 2, 1).reshape(U.C, 192, 3, 3)[:, :191], weight)
    print(f"one-hot convolutions: max |conv2d - selection| {worst:.3e} (float64)")
    assert worst <= 8 * 2.0 ** -53 * 5                              # values below 5 (|N(0, 1)| + |bias|): a few float64 roundings


def test_repack_is_cached_on_pointer_and_version():
    from batrack_amd.frontend import tracker
    conv = torch.nn.Conv2d(191, 128, 3, padding=1)
    a, _ = tracker.packed_conv(conv)
    assert tracker.packed_conv(conv)[0] is a
    with torch.no_grad():
        conv.weight.mul_(2.0)
    b, _ = tracker.packed_conv(conv)
    assert b is not a and torch.equal(b, tracker.pack_weights(conv.weight))
    with pytest.raises(RuntimeError, match="padding"):
        tracker.packed_conv(torch.nn.Conv2d(191, 128, 3, padding=0))


def test_signature_is_the_references():
    from batrack_amd.frontend import tracker
    got = str(inspect.signature(tracker.forward))
    assert got == str(D["signature"])
    assert got == "(self, rgbds, queries, iters=4, feat_init=None, is_train=False)"


def test_install_returns_the_previous_binding_and_is_idempotent():
    from batrack_amd.frontend import tracker
    mod = types.ModuleType("stand_in_tracker")
    old = lambda self, rgbds, queries: None
    mod.MDTracker = type("MDTracker", (), {"forward": old})
    assert tracker.install(mod) is old
    assert mod.MDTracker.forward is tracker.forward
    assert tracker.install(mod) is tracker.forward and mod.MDTracker.forward is tracker.forward


def test_symbols_are_exported_and_sources_listed():
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "batrack_window.h")).read()
    for name in ("bt_window_workspace_bytes", "bt_depth_range", "bt_window_depth", "bt_embed_conv", "bt_feat_sample"):
        assert hasattr(L, name) and name in header, name
    assert "window_fmaps.hip" in _lib.SOURCES and any(h.endswith("batrack_window.h") for h in _lib.HEADERS)
    assert "tracker window" in _lib.ERRORS[_lib.BT_EUNSUPPORTED]
    import batrack_amd.frontend
    assert "tracker.forward" in batrack_amd.frontend.__doc__


def test_abi_refuses_before_launching():
    """Argument checks return their codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    p = ctypes.c_void_p(256)                           # never dereferenced: every call below is refused first
    EINVAL, EUNS, OK = _lib.BT_EINVAL, _lib.BT_EUNSUPPORTED, _lib.BT_OK
    f, big = ctypes.c_float, (1 << 31)
    assert L.bt_window_workspace_bytes() >= 4

    ok = dict(depth=p, T=3, H=8, W=8, st=256, sy=8, sx=1, log=0, ws=p, out=p)
    dr = lambda **k: L.bt_depth_range(*(dict(ok, **k)[n] for n in ok), None)
    for name in ("depth", "ws", "out"):
        assert dr(**{name: None}) == EINVAL, name
    for k in (dict(T=0), dict(H=0), dict(W=-1), dict(st=-1)):
        assert dr(**k) == EINVAL, k
    for k in (dict(T=big), dict(T=1 << 11, H=1 << 10, W=1 << 10), dict(st=big), dict(T=1 << 20, st=1 << 20)):
        assert dr(**k) == EUNS, k

    ok = dict(depth=p, frames=3, S=4, H=8, W=8, st=256, sy=8, sx=1, stride=4, d_near=f(0.5), d_range=f(19.5), Dz=f(2), log=0, ws=p, dmaps=p, zr=p)
    wd = lambda **k: L.bt_window_depth(*(dict(ok, **k)[n] for n in ok), None)
    for name in ("depth", "ws", "dmaps", "zr"):
        assert wd(**{name: None}) == EINVAL, name
    for k in (dict(frames=0), dict(frames=5), dict(S=0), dict(stride=0), dict(stride=16), dict(H=0)):
        assert wd(**k) == EINVAL, k
    for k in (dict(S=big, frames=1), dict(S=1 << 12, H=1 << 12, W=1 << 12, stride=1), dict(H=big), dict(st=big)):
        assert wd(**k) == EUNS, k

    ok = dict(fnet=p, sf=128 * 35, sc=35, sy=7, sx=1, dmaps=p, zr=p, wp=p, bias=p, freqs=p, S=4, frame0=2, F=0, h=5, w=7, C=128, out=p)
    ec = lambda **k: L.bt_embed_conv(*(dict(ok, **k)[n] for n in ok), None)
    assert ec() == OK and ec(frame0=4) == OK                       # F = 0: nothing to launch
    for name in ("fnet", "dmaps", "zr", "wp", "bias", "freqs", "out"):
        assert ec(**{name: None}) == EINVAL, name
    assert ec(wp=ctypes.c_void_p(260)) == EINVAL                    # the packed weights are read 16 bytes at a time
    for k in (dict(h=1), dict(w=1), dict(h=0), dict(S=0), dict(frame0=-1), dict(frame0=3, F=2), dict(F=-1), dict(C=0), dict(sc=-1)):
        assert ec(**k) == EINVAL, k
    for k in (dict(C=64), dict(C=129), dict(C=191), dict(h=big), dict(S=1 << 10, h=1 << 7, w=1 << 7, F=1), dict(F=1, frame0=0, sf=big)):
        assert ec(**k) == EUNS, k

    ok = dict(fmaps=p, S=4, C=128, h=5, w=7, frames=p, xy=p, xs=3, n=0, out=p)
    fs = lambda **k: L.bt_feat_sample(*(dict(ok, **k)[n] for n in ok), None)
    assert fs() == OK
    for name in ("fmaps", "frames", "xy", "out"):
        assert fs(**{name: None}) == EINVAL, name
    for k in (dict(S=0), dict(C=0), dict(h=0), dict(w=0), dict(xs=1), dict(n=-1)):
        assert fs(**k) == EINVAL, k
    for k in (dict(C=64), dict(S=big), dict(S=1 << 10, h=1 << 7, w=1 << 7), dict(n=1 << 24), dict(n=big), dict(xs=big)):
        assert fs(**k) == EUNS, k


def test_operator_schemas():
    ops = _lib.torch_ops(strict=True)
    assert str(ops.depth_range.default._schema) == "batrack_hip::depth_range(Tensor depth, bool use_log_depth) -> Tensor"
    assert str(ops.window_depth.default._schema) == (
        "batrack_hip::window_depth(Tensor depth, int S, int stride, float d_near, float d_range, float dz, bool use_log_depth) -> (Tensor, Tensor)")
    assert str(ops.embed_conv.default._schema) == (
        "batrack_hip::embed_conv(Tensor fnet_maps, Tensor dmaps, Tensor zrange, Tensor wpacked, Tensor bias, Tensor freqs, int frame0, "
        "Tensor(a!) out) -> ()")
    assert str(ops.feat_sample.default._schema) == "batrack_hip::feat_sample(Tensor fmaps, Tensor frames, Tensor xy) -> Tensor"


def test_cpu_tensors_raise():
    from batrack_amd.frontend import tracker
    z = torch.zeros
    conv = torch.nn.Conv2d(191, 128, 3, padding=1)
    with pytest.raises(RuntimeError, match="GPU"):
        tracker.depth_range(z(2, 8, 8))
    with pytest.raises(RuntimeError, match="GPU"):
        tracker.window_depth(z(2, 8, 8), 2, 4, 0.5, 20.0, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        tracker.embed_conv(z(2, 128, 5, 7), z(2, 5, 7), z(2), 0, conv, U.FREQS)
    with pytest.raises(RuntimeError, match="GPU"):
        tracker.sample_features(z(2, 128, 5, 7), z(3, dtype=torch.int32), z(3, 2))
    me = U.StandIn("C", torch.float32, "cpu", U.embed3d_stand_in())
    T = U.case_tensors("C")
    with pytest.raises(RuntimeError, match="GPU"):
        tracker.forward(me, T["rgbds"], T["queries"])
    with pytest.raises(RuntimeError, match="inference only"):
        tracker.forward(me, T["rgbds"], T["queries"], is_train=True)
    ops = _lib.torch_ops(strict=True)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.feat_sample(z(2, 128, 5, 7), z(3, dtype=torch.int32), z(3, 2))


def test_import_surface():
    """Importing the module loads no native library and no oracle."""
    code = ("import sys; import batrack_amd.frontend.tracker; from batrack_amd import _lib; "
            "assert 'oracle' not in sys.modules and _lib._lib is None and _lib._torch_ops is None; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
