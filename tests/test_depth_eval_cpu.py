"""CPU half of the global-alignment stage's output and depth metrics: the reference's fixtures (tests/golden/depth_eval.npz,
made by the unmodified reference) against the numpy restatement in tests/depth_util.py; the `model.*` import surface of
integration/global_refine against the recorded signatures; the arguments that must raise without touching a GPU."""
import ctypes
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from batrack_amd import _lib
from depth_util import np_depth_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = dict(np.load(os.path.join(ROOT, "tests", "golden", "depth_eval.npz")))
NAMES = [str(n) for n in D["ce.names"]]
SCALING = {0: "none", 1: "median", 2: "lstsq"}


def case(name):
    kg, kp, km = (str(k) for k in D[f"ce.{name}.inputs"])
    dmin, dmax = D[f"ce.{name}.limits"]
    return D[f"ce.in.{kg}"], D[f"ce.in.{kp}"], D[f"ce.in.{km}"], float(dmin), float(dmax), SCALING[int(D[f"ce.{name}.scaling"])]


@pytest.mark.parametrize("name", NAMES)
def test_fixtures_agree_with_the_numpy_restatement(name):
    gt, pred, mask, dmin, dmax, scaling = case(name)
    r, ref, aux = np_depth_metrics(gt, pred, mask, dmin, dmax, scaling), D[f"ce.{name}.metrics"], D[f"ce.{name}.aux"]
    assert r[8] == aux[0]
    if scaling == "median":
        assert r[9] == aux[1]
    np.testing.assert_allclose(r[:5], ref[:5], rtol=1e-12)
    assert np.abs(r[5:8] - ref[5:]).max() <= (1.0 / aux[0] if scaling == "lstsq" else 0.0)


def test_fixture_cases_cover_what_they_claim():
    counts = {n: int(D[f"ce.{n}.aux"][0]) for n in NAMES}
    for s in ("median", "lstsq", "none"):
        assert counts[f"{s}_odd"] % 2 == 1 and counts[f"{s}_even"] % 2 == 0
    gt, pred, mask, dmin, dmax, _ = case("median_odd")
    v = mask & (gt > dmin) & (gt < dmax)
    ratio = D["ce.median_odd.aux"][1]
    assert (pred[v] * ratio < dmin).any() and (pred[v] * ratio > dmax).any()          # both clamps are exercised
    tg = case("median_ties")[0]
    assert np.unique(tg).size < tg.size / 20                                           # heavy ties
    assert len(D["loop.free.lr"]) == 20 and D["sd.g35.frame_shifts_"].any()


SURFACE = r"""
import inspect, json, sys
from model.refine_net import RefineNet
from model.trainer import global_alignment_loop, cosine_schedule, linear_schedule
from model.utils import eval_depth, eval_depth_metric, compute_errors
import batrack_amd.global_refine as g, batrack_amd.evaluation as e
assert RefineNet is g.RefineNet and global_alignment_loop is g.global_alignment_loop and eval_depth is e.eval_depth
s = lambda f: str(inspect.signature(f))
print(json.dumps({"RefineNet.__init__": s(RefineNet.__init__), "global_alignment_loop": s(global_alignment_loop),
                  "cosine_schedule": s(cosine_schedule), "linear_schedule": s(linear_schedule), "eval_depth": s(eval_depth),
                  "eval_depth_metric": s(eval_depth_metric), "compute_errors": s(compute_errors)}))
"""


def test_model_forwards_import_with_the_reference_signatures():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "integration", "global_refine"), ROOT]))
    r = subprocess.run([sys.executable, "-c", SURFACE], capture_output=True, text=True, env=env, cwd="/tmp")
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "signatures_global_refine.json")))
    want = dict(ref["refine_net"], **ref["trainer"], **ref["utils"])
    assert got == want


def test_cpu_tensors_and_unported_scalings_raise():
    from batrack_amd.evaluation import compute_errors, eval_depth_metric
    with pytest.raises(RuntimeError, match="GPU"):
        compute_errors(torch.ones(8), torch.ones(8), 0.1, 10.0)
    with pytest.raises(RuntimeError, match="GPU"):
        eval_depth_metric(np.ones(8), {"final": torch.ones(8)}, None)
    for s in ("lad", "la2d"):
        with pytest.raises(NotImplementedError, match="not"):
            compute_errors(np.ones(8), np.ones(8), 0.1, 10.0, scaling=s)


def test_schedules_are_the_reference_formulas():
    from batrack_amd.global_refine import cosine_schedule, linear_schedule
    np.testing.assert_array_equal([cosine_schedule(n / 20, 1e-2, 1e-6) for n in range(20)], D["loop.free.lr"])
    assert linear_schedule(0.25, 1e-2, 1e-6) == 1e-2 + (1e-6 - 1e-2) * 0.25
    with pytest.raises(AssertionError):
        cosine_schedule(1.5, 1e-2, 1e-6)


def test_abi_refuses_before_launching():
    """Size and argument checks return codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    p = ctypes.c_void_p(256)                           # never dereferenced: every call below is refused first
    assert L.bt_depth_metrics_workspace_bytes(1 << 20) > 0
    assert L.bt_depth_metrics_workspace_bytes(-1) == _lib.BT_EINVAL
    assert L.bt_depth_metrics_workspace_bytes(1 << 31) == _lib.BT_EUNSUPPORTED
    assert L.bt_depth_metrics(p, p, None, 1 << 31, 0.1, 10.0, 1, p, p, None) == _lib.BT_EUNSUPPORTED
    assert L.bt_depth_metrics(p, p, None, 16, 0.1, 10.0, 3, p, p, None) == _lib.BT_EINVAL
    assert L.bt_depth_metrics(p, p, None, -1, 0.1, 10.0, 1, p, p, None) == _lib.BT_EINVAL
    assert L.bt_depth_metrics(None, p, None, 16, 0.1, 10.0, 1, p, p, None) == _lib.BT_EINVAL
    assert L.bt_ga_scaled_dmaps(p, p, p, p, 2, 4, 8193, 8, 8, None) == _lib.BT_EUNSUPPORTED
    assert L.bt_ga_scaled_dmaps(p, p, p, p, 1 << 16, 4, 4, 1 << 16, 8, None) == _lib.BT_EUNSUPPORTED
    assert L.bt_ga_scaled_dmaps(p, p, p, p, 0, 4, 4, 8, 8, None) == _lib.BT_EINVAL
    assert L.bt_ga_scaled_dmaps(None, p, p, p, 2, 4, 4, 8, 8, None) == _lib.BT_EINVAL
