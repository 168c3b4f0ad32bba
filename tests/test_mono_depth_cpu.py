"""CPU half of the mono-depth alignment (main/mono_depth/get_mono_depth.py:21-150, include/batrack_depth.h bt_mono_align): the
numpy restatement (mono_util.py) against the unmodified reference's outputs (tests/golden/mono_depth.npz), what the fixture's
cases cover, the C ABI's refusals and workspace sizes (nothing is launched), align_mono_depth's argument checks, K, the image
size, and the names and signatures of integration/mono_depth/get_mono_depth.py."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from batrack_amd import _lib
from mono_util import percentile_gamma, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = dict(np.load(os.path.join(ROOT, "tests", "golden", "mono_depth.npz")))
CASES = [str(n) for n in D["names"]]


def pairs(case):
    d, m = D[f"{case}.mono"], D[f"{case}.metric"]
    T = min(len(d), len(m))
    return d[:T], m[:T]


@pytest.mark.parametrize("case", CASES)
def test_restatement_is_the_reference(case):
    d, m = pairs(case)
    depth, *_ = restate(d, m)
    ref = D[f"{case}.depth"]
    assert depth.dtype == ref.dtype == m.dtype and depth.shape == ref.shape
    assert np.array_equal(depth, ref, equal_nan=True)


def test_fixture_cases_cover_what_they_claim():
    size = lambda c: D[f"{c}.metric"].shape[1] * D[f"{c}.metric"].shape[2]
    assert size("even") % 2 == 0 and size("odd") % 2 == 1 and size("odd_f64") % 2 == 1
    assert D["f64.metric"].dtype == D["odd_f64.metric"].dtype == np.float64 and D["even.metric"].dtype == np.float32
    assert len(D["single.metric"]) == 1 and len(D["mismatch.mono"]) == 5 and len(D["mismatch.metric"]) == 4
    gammas = {c: percentile_gamma(D[f"{c}.depth"].size, D[f"{c}.metric"].dtype.type) for c in CASES}
    assert any(g >= 0.5 for g in gammas.values()) and any(g < 0.5 for g in gammas.values())
    d, m = D["even.mono"], D["even.metric"]
    f2 = np.float32(0.02)
    for dv in (np.nextafter(f2, np.float32(0)), f2, np.nextafter(f2, np.float32(1))):
        for mv in (np.nextafter(np.float32(2), np.float32(0)), np.float32(2), np.nextafter(np.float32(2), np.float32(3))):
            assert ((d == dv) & (m == mv)).any()
    assert (d[2] < 0.01).mean() > 0.5                                          # a sky-dominated frame
    for c in ("even", "f64"):
        m = D[f"{c}.metric"]
        assert (m == 0).any() and np.isposinf(m).any() and np.isneginf(m).any() and (m < 0).any()
    _, s, sh, _, k = restate(*pairs("ties"))
    p = s * sh
    dist = np.abs(p - np.median(p))
    assert k == 1 and dist[1] == dist[2] == dist.min()                         # a tie in argmin: the first index
    assert np.unique(D["ties.mono"]).size < 16
    for c in CASES:                                                            # negative ratios
        d, m = pairs(c)
        with np.errstate(all="ignore"):
            g = 1 / (m[0] + m.dtype.type(1e-8))
            r = (g - np.median(g) + m.dtype.type(1e-8)) / (d[0] - np.median(d[0]) + np.float32(1e-8))
        assert (r < 0).any()
    assert np.isnan(D["nan_metric.metric"][1]).any() and np.isfinite(D["nan_metric.depth"]).all()
    _, s, _, _, k = restate(*pairs("nan_metric"))
    assert np.isnan(s[1]) and k == 0
    assert np.isnan(D["nan_mono.mono"][1]).any() and np.isnan(D["nan_mono.depth"]).all()


def test_abi_refuses_before_launching():
    """Argument and size checks return codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    F32, F64 = _lib.BT_DEPTH_F32, _lib.BT_DEPTH_F64
    wsb = L.bt_mono_align_workspace_bytes
    assert wsb(50, 480 * 854, F32) == wsb(50, 480 * 854, F64) == wsb(50, 1, F32) > 50 * 4096
    assert wsb(64, 7, F32) > wsb(50, 7, F32) and wsb(1, 1, F64) > 0 and wsb(1, 1, F64) % 256 == 0
    assert wsb(0, 8, F32) == wsb(1, 0, F32) == wsb(1, 8, 2) == wsb(-1, 8, F64) == _lib.BT_EINVAL
    assert wsb(1, (1 << 31) - 1, F32) > 0 and wsb((1 << 31) - 1, 1, F64) > 0
    assert wsb(1, 1 << 31, F32) == wsb(2, 1 << 30, F64) == wsb(1 << 40, 1 << 40, F32) == _lib.BT_EUNSUPPORTED
    base = 1 << 32                                                             # never dereferenced
    mono, metric, out, ws = base, base + (1 << 24), base + (2 << 24), base + (3 << 24)

    def call(mono=mono, metric=metric, T=4, hw=64, dt=F64, out=out, fs=None, fc=None, al=None, k=None, ws=ws):
        return L.bt_mono_align(mono, metric, T, hw, dt, out, fs, fc, al, k, ws, None)
    for kw in ({"T": 0}, {"hw": 0}, {"T": -3}, {"dt": 2}, {"mono": None}, {"metric": None}, {"out": None}, {"ws": None}):
        assert call(**kw) == _lib.BT_EINVAL, kw
    assert call(T=1 << 20, hw=1 << 11) == _lib.BT_EUNSUPPORTED                 # 2^31 pixels
    assert call(T=1, hw=1 << 31, dt=F32) == _lib.BT_EUNSUPPORTED
    assert call(T=1 << 20, hw=1 << 11, mono=None) == _lib.BT_EINVAL             # the argument check comes first
    n = 4 * 64
    for kw in ({"out": metric + 8 * n - 8}, {"out": mono + 4 * n - 8}, {"out": metric - 8 * n + 8}, {"fs": metric + 16},
               {"fc": mono}, {"al": metric + 8 * n - 8}, {"k": mono + 8}, {"ws": metric + 64}, {"ws": out + 8 * n - 16},
               {"fs": ws + 256}):
        assert call(**kw) == _lib.BT_EINVAL, kw                                # an output (or the workspace) meets an input
    for kw in ({"ws": ws + 8}, {"out": out + 4}, {"metric": metric + 4}, {"mono": mono + 2}, {"k": base + (5 << 24) + 4}):
        assert call(**kw) == _lib.BT_EINVAL, kw                                # misaligned


def test_align_mono_depth_argument_checks():
    from batrack_amd.mono_depth import align_mono_depth
    d32, m32 = torch.rand(2, 3, 4), torch.rand(2, 3, 4) + 1
    with pytest.raises(RuntimeError, match="GPU"):
        align_mono_depth(d32, m32)
    with pytest.raises(RuntimeError, match="GPU"):
        align_mono_depth(d32.double(), m32.double())
    for bad in (m32.half(), m32.to(torch.int32), m32.bfloat16()):
        with pytest.raises(TypeError):
            align_mono_depth(d32, bad)
    with pytest.raises(TypeError):
        align_mono_depth(d32.to(torch.int64), m32)
    with pytest.raises(TypeError):
        align_mono_depth(d32.numpy(), m32)
    with pytest.raises(ValueError):
        align_mono_depth(torch.rand(2, 3, 5), m32)                             # another resolution
    with pytest.raises(ValueError):
        align_mono_depth(torch.rand(3, 3, 4), m32)                             # another frame count
    with pytest.raises(ValueError):
        align_mono_depth(d32[0], m32[0])                                       # not [T,H,W]


@pytest.mark.parametrize("case", CASES)
def test_K_is_the_reference(case):
    from batrack_amd.mono_depth import intrinsics_to_fov, scene_intrinsics
    m, intr = D[f"{case}.metric"], D[f"{case}.intrinsics"]
    fovs = [intrinsics_to_fov(k, x) for k, x in zip(intr, m)][:len(D[f"{case}.depth"])]
    assert all(f.dtype == intr.dtype for f in fovs)
    K = scene_intrinsics(fovs, *D[f"{case}.image_hw"].tolist())
    ref = D[f"{case}.K"]
    assert K.dtype == ref.dtype and np.array_equal(K.view(np.uint64), ref.view(np.uint64))


def test_image_size_is_cv2s_and_refuses_a_rotated_image(tmp_path):
    from PIL import Image
    from batrack_amd.mono_depth import _image_size
    Image.new("RGB", (40, 30)).save(tmp_path / "a.png")
    assert _image_size(str(tmp_path / "a.png")) == (30, 40)
    ex = Image.Exif()
    ex[0x0112] = 1
    Image.new("RGB", (40, 30)).save(tmp_path / "b.jpg", exif=ex)
    assert _image_size(str(tmp_path / "b.jpg")) == (30, 40)
    ex[0x0112] = 6
    Image.new("RGB", (40, 30)).save(tmp_path / "c.jpg", exif=ex)
    with pytest.raises(ValueError, match="orientation"):
        _image_size(str(tmp_path / "c.jpg"))


SURFACE = r"""
import inspect, json, sys
import get_mono_depth as g
import batrack_amd.mono_depth as m
names = ("intrinsics_to_fov", "align_depth", "align_davis_demo")
assert all(getattr(g, n) is getattr(m, n) for n in names)
print(json.dumps({n: str(inspect.signature(getattr(g, n))) for n in names}))
"""


def test_integration_forwards_the_reference_names_and_signatures():
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "integration", "mono_depth"))
    r = subprocess.run([sys.executable, "-c", SURFACE], capture_output=True, text=True, env=env, cwd="/tmp")
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == json.loads(str(D["signatures"]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "integration", "mono_depth", "get_mono_depth.py"), "--help"],
                       capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and all(a in r.stdout for a in ("--depth_dir", "--data_dir", "--save_name")), r.stderr
