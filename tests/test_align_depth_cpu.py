"""CPU half of the depth-map alignment (main/global_refine/model/utils.py:268-312, include/batrack_depth.h
bt_align_depth_maps): the host restatement `_align_depth_maps` against the unmodified reference's outputs
(tests/golden/align_depth.npz), what the fixture's cases cover, the C ABI's refusals (nothing is launched), and the
`model.utils` name of integration/global_refine."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from align_util import host_align_stats
from batrack_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = dict(np.load(os.path.join(ROOT, "tests", "golden", "align_depth.npz")))
NAMES = [str(n) for n in D["names"]]


def bits(a):
    return np.ascontiguousarray(a).view(f"u{a.dtype.itemsize}")


@pytest.mark.parametrize("name", NAMES)
def test_host_restatement_is_the_reference_bit_for_bit(name):
    from batrack_amd.global_refine import _align_depth_maps
    maps, ref = D[f"{name}.maps"], D[f"{name}.aligned"]
    with np.errstate(all="ignore"):
        out = _align_depth_maps(maps)
    assert out.dtype == ref.dtype and out.shape == ref.shape
    np.testing.assert_array_equal(bits(out), bits(ref))
    a, _, overlap, _ = host_align_stats(maps[..., 0])
    np.testing.assert_array_equal(bits(a), bits(ref[..., 0]))
    skipped = np.flatnonzero(overlap < 100)
    np.testing.assert_array_equal(skipped[skipped > 0], D[f"{name}.skipped"])          # the frames the reference printed
    np.testing.assert_array_equal(overlap[skipped[skipped > 0]], D[f"{name}.printed"])


def test_fixture_cases_cover_what_they_claim():
    for dt in ("float32", "float64"):
        assert any(f"{c}.{dt}.c2" in NAMES for c in ("chain", "underflow"))
        _, s, ov, un = host_align_stats(D[f"chain.{dt}.c1.maps"][..., 0])
        assert ov[1] == 100 and ov[2] == 99 and np.isnan(s[2]) and np.isfinite(s[3])      # threshold, skipped, the frame after
        assert {int(c) % 2 for c in ov[1:] if c >= 100} == {0, 1} and {int(u) % 2 for u in un[3:]} == {0, 1}
        maps = D[f"chain.{dt}.c1.maps"][..., 0]
        assert np.unique(maps[4][maps[4] > 0]).size == 3                                   # heavy ties
        assert np.isposinf(maps).any() and np.isnan(maps).any() and (maps == 0).any() and (maps < 0).any()
        _, s, ov, un = host_align_stats(D[f"empty_past.{dt}.c1.maps"][..., 0])
        assert ov[1] == 0 and ov[2] == un[2] > 100                                          # frame 2's past set is empty
        m, a = D[f"underflow.{dt}.c1.maps"][..., 0], D[f"underflow.{dt}.c1.aligned"][..., 0]
        tiny = np.finfo(a.dtype).tiny
        assert ((m[1] > 0) & (a[1] == 0)).sum() > 100 and ((a[1] > 0) & (a[1] < tiny)).any()
        m, a = D[f"overflow.{dt}.c1.maps"][..., 0], D[f"overflow.{dt}.c1.aligned"][..., 0]
        _, s, ov, _ = host_align_stats(m)
        assert (np.isfinite(m[1]) & np.isinf(a[1])).sum() == 200
        assert s[2] == 0 and np.isposinf(s[4]) and np.isnan(s[5]) and ov[3] == 0 and ov[6] == 0


def test_abi_refuses_before_launching():
    """Size and argument checks return codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    F32, F64 = _lib.BT_DEPTH_F32, _lib.BT_DEPTH_F64
    p, q, w = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 28), ctypes.c_void_p(1 << 12)   # never dereferenced
    assert L.bt_align_depth_maps_workspace_bytes(436 * 1024, F64) > 0
    assert L.bt_align_depth_maps_workspace_bytes(436 * 1024, F32) > 0
    assert L.bt_align_depth_maps_workspace_bytes(0, F64) == _lib.BT_EINVAL
    assert L.bt_align_depth_maps_workspace_bytes(16, 2) == _lib.BT_EINVAL
    assert L.bt_align_depth_maps_workspace_bytes(1 << 30, F32) == _lib.BT_EUNSUPPORTED
    assert L.bt_align_depth_maps_workspace_bytes((1 << 30) - 1, F32) > 0
    call = lambda maps=p, out=q, T=4, hw=64, dt=F64, sc=None, ov=None, ws=w: L.bt_align_depth_maps(maps, out, T, hw, dt, sc, ov, ws, None)
    assert call(T=0) == _lib.BT_EINVAL
    assert call(hw=0) == _lib.BT_EINVAL
    assert call(dt=2) == _lib.BT_EINVAL
    assert call(maps=None) == _lib.BT_EINVAL
    assert call(out=None) == _lib.BT_EINVAL
    assert call(ws=None) == _lib.BT_EINVAL
    assert call(hw=1 << 30) == _lib.BT_EUNSUPPORTED
    assert call(hw=1 << 30, dt=F32) == _lib.BT_EUNSUPPORTED
    assert call(T=1 << 40, hw=(1 << 30) - 1) == _lib.BT_EUNSUPPORTED                   # T * hw * 8 bytes overflows
    nb = 4 * 64 * 8
    assert call(out=ctypes.c_void_p((1 << 20) + 8)) == _lib.BT_EINVAL                  # a partial overlap of maps and aligned
    assert call(out=ctypes.c_void_p((1 << 20) + nb - 8)) == _lib.BT_EINVAL
    assert call(out=ctypes.c_void_p((1 << 20) - nb + 8)) == _lib.BT_EINVAL


SURFACE = r"""
import inspect, json
import numpy as np
from model.utils import align_depth_maps
import batrack_amd.global_refine as g
assert align_depth_maps is g.align_depth_maps
sig = inspect.signature(align_depth_maps)
pos = [n for n, p in sig.parameters.items() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
extra_have_defaults = all(p.default is not p.empty for n, p in sig.parameters.items() if n not in pos)
half = np.ones((3, 4, 5, 1), np.float16)
print(json.dumps({"positional": pos, "extra_have_defaults": extra_have_defaults,
                  "host_dtype": str(align_depth_maps(half).dtype)}))
"""


def test_model_utils_forwards_align_depth_maps_with_the_reference_signature():
    """The reference calls align_depth_maps(depth_maps) (refine_net.py, align_depth=True): one positional parameter of that
    name; return_stats is keyword-only with a default.  Dtypes other than float32 / float64 keep the host function (no GPU)."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "integration", "global_refine"), ROOT]))
    r = subprocess.run([sys.executable, "-c", SURFACE], capture_output=True, text=True, env=env, cwd="/tmp")
    assert r.returncode == 0, r.stderr
    import json
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == {"positional": ["depth_maps"], "extra_have_defaults": True, "host_dtype": "float16"}
