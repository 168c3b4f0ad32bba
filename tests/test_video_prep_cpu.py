"""CPU half of the tracker's input preparation (bt_frame_prep in include/batrack_video.h, batrack_amd/frontend/video.py): the
reference's fixture (tests/golden/video_prep.npz, made by its unmodified `_compute_sparse_tracks`) against the torch
restatement in tests/video_util.py; the input digests, the exact source coordinate, the window cache's bookkeeping with
stand-ins, the ABI's refusals and the import surface — none of which touch a GPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import video_util as U
from batrack_amd import _lib

D = dict(np.load(U.GOLD))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def video():
    from batrack_amd.frontend import video
    return video


@pytest.fixture(scope="module")
def restated():
    runs = {}
    for c in U.CASES:
        for dtype in (torch.float32, torch.float64):
            t = U.case_tensors(c, dtype)
            me = U.StandIn(c, dtype, "cpu")
            ret = U.compute_sparse_tracks(me, t["rgbds"], t["queries"])
            runs[c, dtype] = dict(rgbds=me.seen[0]["rgbds"][0], queries=me.seen[0]["queries"], tracks=ret[0], depths=ret[1],
                                  visibilities=ret[2], dynamic_e=ret[3]["dynamic_e"])
    return runs


@pytest.mark.parametrize("c", list(U.CASES))
def test_generator_reproduces_the_fixtures_inputs(c):
    d = U.make_inputs(**U.CASES[c])
    assert set(d) == set(U.INPUTS)
    for name, v in d.items():
        assert np.array_equal(U.digest(v), D[f"{c}.digest.{name}"]), name
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
    depth = d["rgbds"][0, :, 3]
    assert (depth == 0).any() and ((depth > 0) & (depth < 0.01)).any() and ((depth > 0.01) & (depth < 0.011001)).any()
    assert str(D["signature"]) == "(self, rgbds, queries)"


@pytest.mark.parametrize("c", list(U.CASES))
def test_float64_restatement_reproduces_the_float64_run(c, restated):
    if c not in U.EXACT64:                                        # 61 x 97: the reference's float64 COORDINATE is rounded (video_util.CASES)
        got, want = restated[c, torch.float64]["rgbds"].numpy(), D[f"{c}.f64.rgbds"]
        assert 1e-12 < np.abs(got - want).max() <= 255 * 2.0 ** -45                # 2 ulp (2^-46 each) of a coordinate below 128, times a colour step
        for name in ("queries",) + U.RETURNS:
            assert np.abs(restated[c, torch.float64][name].numpy() - D[f"{c}.f64.{name}"]).max() <= 1e-12, name
        return
    for name in ("rgbds", "queries") + U.RETURNS:
        got, want = restated[c, torch.float64][name].numpy(), D[f"{c}.f64.{name}"]
        assert got.shape == want.shape and want.dtype == np.float64, name
        assert np.abs(got - want).max() <= 1e-12, (name, np.abs(got - want).max())


@pytest.mark.parametrize("c", list(U.CASES))
def test_float32_restatement_is_within_twice_the_gate_of_the_float64_run(c, restated):
    got, gate = restated[c, torch.float32]["rgbds"], float(D[f"gate.{c}"])
    assert got.dtype == torch.float32
    err = float(np.abs(got.numpy().astype(np.float64) - D[f"{c}.f64.rgbds"]).max())
    print(f"case {c}: max |restatement32 - float64 run| {err:.3e}, gate {gate:.3e}")
    if c in U.RESIZING:
        assert 0 < gate < 5e-3 and err <= 2 * gate
    else:
        assert gate == 0 and np.array_equal(got.numpy(), D[f"{c}.rgbds"]) and np.array_equal(got, U.case_tensors(c)["rgbds"][0])
    # downstream of the stand-in network the float32 run is the reference's bit for bit
    for name in ("queries",) + U.RETURNS:
        assert np.array_equal(restated[c, torch.float32][name].numpy(), D[f"{c}.{name}"]), name


def test_taps_are_the_exact_coordinate():
    from fractions import Fraction
    for n_in, n_out in ((23, 24), (97, 40), (436, 384), (7, 1), (1, 5), (5, 5)):
        i0, i1, l0, l1 = U.taps(n_in, n_out, torch.float64)
        for o in range(n_out):
            src = max(Fraction(0), (Fraction(2 * o + 1, 2)) * Fraction(n_in, n_out) - Fraction(1, 2))
            assert int(i0[o]) == src.numerator // src.denominator and int(i1[o]) == min(int(i0[o]) + 1, n_in - 1)
            assert float(l1[o]) == float(src - int(i0[o])) and float(l0[o]) == 1 - float(l1[o])
    assert bool((U.taps(9, 9, torch.float32)[3] == 0).all())                                  # the identity size: no fraction at all


def test_window_frames_bookkeeping_with_stand_ins(video, monkeypatch):
    """Slots, order and call counts on the CPU: `prepare_frames` and the GPU check are replaced by stand-ins that tag each
    frame, so nothing is launched."""
    calls = []

    def fake_prepare(image, depth, size, normalise, log, out=None):
        calls.append(("prepare", image.shape[0], normalise))
        out[:] = image[:, :1, :1, :1].float()
        return out, torch.stack([depth[:, 0, 0], depth[:, 0, 0] + 1], -1)

    def fnet(x):
        calls.append(("fnet", x.shape[0]))
        return x[:, :1, :2, :3] * 10

    monkeypatch.setattr(video, "prepare_frames", fake_prepare)
    monkeypatch.setattr(video, "_check_frames", lambda image, depth, what: (image, depth))
    wf = video.WindowFrames(4, fnet, size=(8, 12))
    assert len(wf) == 0
    with pytest.raises(RuntimeError, match="no frame"):
        wf.window()
    tag = 0
    for burst in (1, 2, 5, 1, 1, 1, 3, 1, 1, 4, 1):
        for __ in range(burst):
            tag += 1
            wf.push(torch.full((3, 5, 7), float(tag)), torch.full((5, 7), float(tag)))
        assert len(wf) == min(4, tag)
        del calls[:]
        rgbd, fmaps, drange = wf.window()
        new = min(burst, 4)
        assert calls == [("prepare", new, True), ("fnet", new)]
        want = list(range(max(1, tag - 3), tag + 1))
        assert rgbd.shape == (len(want), 4, 8, 12) and fmaps.shape == (len(want), 1, 2, 3)
        assert rgbd[:, 0, 0, 0].tolist() == want and (fmaps[:, 0, 0, 0] / 10).tolist() == want
        assert drange.tolist() == [want[0], want[-1] + 1]
        del calls[:]
        again = wf.window()
        assert calls == [] and all(torch.equal(a, b) for a, b in zip(again, (rgbd, fmaps, drange)))
    wf.clear()
    assert len(wf) == 0


def test_cpu_tensors_and_bad_arguments_raise(video):
    t = U.case_tensors("same")
    img, dep = t["rgbds"][0, :, :3], t["rgbds"][0, :, 3]
    with pytest.raises(RuntimeError, match="GPU"):
        video.prepare_frames(img, dep)
    with pytest.raises(RuntimeError, match="GPU"):
        video.compute_sparse_tracks(U.StandIn("same", torch.float32, "cpu"), t["rgbds"], t["queries"])
    with pytest.raises(RuntimeError, match="GPU"):
        video.WindowFrames(4, lambda x: x).push(img[0], dep[0])
    with pytest.raises(RuntimeError, match=r"\[3, H, W\]"):
        video.WindowFrames(4, lambda x: x).push(img, dep)
    ops = _lib.torch_ops(strict=True)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_prep(img, dep, True, False, torch.zeros(64, dtype=torch.int32), torch.zeros(2, 4, 24, 40), torch.zeros(2, 2))


def test_symbols_are_exported_and_sources_listed(video):
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "batrack_video.h")).read()
    for name in ("bt_frame_prep_workspace_bytes", "bt_frame_prep"):
        assert hasattr(L, name) and name in header, name
    for name, value in (("VEC", U.VEC), ("TILE", U.TILE), ("MAX_BLOCKS", U.MAX_BLOCKS), ("GRID_FRAMES", U.GRID_FRAMES)):
        assert f"#define BT_VIDEO_{name} {value} " in header, name
    assert "video_prep.hip" in _lib.SOURCES and "minmax_reduce.hpp" in _lib.HEADERS
    assert any(h.endswith("batrack_video.h") for h in _lib.HEADERS)
    assert "frame preparation" in _lib.ERRORS[_lib.BT_EUNSUPPORTED]
    src = {f: open(os.path.join(_lib.CSRC, f)).read() for f in ("video_prep.hip", "window_fmaps.hip", "minmax_reduce.hpp")}
    for f in ("video_prep.hip", "window_fmaps.hip"):                # one copy of the reduction, in the header
        assert '#include "minmax_reduce.hpp"' in src[f] and "minmax_finish(" in src[f] and "__device__ inline void minmax_finish" not in src[f]
        assert "atomicAdd" not in src[f]
    assert src["minmax_reduce.hpp"].count("void minmax_finish(") == 1
    import batrack_amd.frontend
    from batrack_amd.frontend import tracker
    for name in ("prepare_frames", "compute_sparse_tracks", "WindowFrames", "install"):
        assert hasattr(video, name) and f"video.{name}" in batrack_amd.frontend.__doc__, name
    assert hasattr(tracker, "forward_frames") and "tracker.forward_frames" in batrack_amd.frontend.__doc__
    assert str(inspect.signature(video.compute_sparse_tracks)) == str(D["signature"])
    assert str(inspect.signature(tracker.forward_frames)) == "(self, frames, queries, iters=4)"
    assert str(inspect.signature(video.prepare_frames)) == "(image, depth, size=(384, 512), normalise=True, use_log_depth=False, out=None)"
    ops = _lib.torch_ops(strict=True)
    assert str(ops.frame_prep.default._schema) == ("batrack_hip::frame_prep(Tensor image, Tensor depth, bool normalise, bool use_log_depth, "
                                                    "Tensor(a!) workspace, Tensor(b!) rgbd, Tensor(c!) drange) -> ()")


def test_install_rebinds_and_returns_the_previous_method(video):
    import types
    mod = types.SimpleNamespace(BATRACK=type("BATRACK", (), {"_compute_sparse_tracks": lambda self, rgbds, queries: "old"}))
    previous = video.install(mod)
    assert previous(None, None, None) == "old" and mod.BATRACK._compute_sparse_tracks is video.compute_sparse_tracks


def test_abi_refuses_before_any_hip_call():
    """Argument checks return their codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    EINVAL, EUNS, OK = _lib.BT_EINVAL, _lib.BT_EUNSUPPORTED, _lib.BT_OK
    P, big = 256, 1 << 31                                          # never dereferenced: every call below is refused first

    def call(image=P, u8=0, si=None, depth=P, sd=None, F=2, H=5, W=7, oh=4, ow=6, ws=P, out=P, dr=P):
        si = si or (3 * H * W, H * W, W, 1)
        sd = sd or (H * W, W, 1)
        return L.bt_frame_prep(image, u8, *si, depth, *sd, F, H, W, oh, ow, 1, 0, ws, out, dr, None)

    assert L.bt_frame_prep_workspace_bytes(12, 384, 512) == U.workspace_bytes(12, 384, 512) == 48 + 12 * 192 * 8
    assert L.bt_frame_prep_workspace_bytes(1, 1, 1) == 16 + 8 and L.bt_frame_prep_workspace_bytes(5, 3, 9) == 32 + 5 * 8
    assert L.bt_frame_prep_workspace_bytes(1, 2048, 2048) == 16 + U.MAX_BLOCKS * 8
    for bad in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, -1), (big, 1, 1), (1, big, 1), (1, 1, big), (1, 1 << 15, 1 << 14), (1 << 29, 1, 1)):
        assert L.bt_frame_prep_workspace_bytes(*bad) == 0, bad

    # ---- BT_EINVAL
    for name in ("image", "depth", "ws", "out", "dr"):
        assert call(**{name: None}) == EINVAL, name
    for k in (dict(F=-1), dict(H=0), dict(W=0), dict(oh=0), dict(ow=0), dict(H=-2), dict(ow=-2)):
        assert call(**k) == EINVAL, k
    for i in range(4):
        si = [105, 35, 7, 1]
        si[i] = -1
        assert call(si=tuple(si)) == EINVAL, i
    for i in range(3):
        sd = [35, 7, 1]
        sd[i] = -1
        assert call(sd=tuple(sd)) == EINVAL, i

    # ---- BT_EUNSUPPORTED
    for k in (dict(F=big), dict(H=big), dict(W=big), dict(oh=big), dict(ow=big), dict(oh=1 << 15, ow=1 << 14), dict(F=1 << 20, oh=32, ow=16),
              dict(H=1 << 15, W=1 << 15), dict(si=(big, 35, 7, 1)), dict(si=(105, big, 7, 1)), dict(si=(105, 35, big, 1)), dict(si=(105, 35, 7, big)),
              dict(sd=(big, 7, 1)), dict(sd=(35, big, 1)), dict(sd=(35, 7, big)), dict(si=(105, 1 << 30, 7, 1)), dict(sd=((1 << 31) - 1, 7, 1))):
        assert call(**k) == EUNS, k

    # ---- nothing to do
    assert call(F=0) == OK
    assert call(F=0, si=(105, 35, 7, big)) == EUNS and call(F=0, out=None) == EINVAL       # refused even then
