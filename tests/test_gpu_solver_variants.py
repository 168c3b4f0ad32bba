"""-m gpu: every reduced-system solver variant, and the persistent variant of the Jacobian kernel, give the
reference's pose update.

The library picks the variant from the system's size (ba_step.cpp: plan_route; the kernels are in ba_solve.hip): the barrier-free double LDS kernel (default where it applies), the
one-phase-per-level kernel with a barrier per level, the two-phase double LDS kernel (levels wider than two columns), the float LDS kernel and the global-memory kernel
(systems too large for LDS).  The environment switches that force a variant are read once per
process, so each case runs in its own interpreter."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
from gpu_util import HipProblem, rel
from batrack_amd import graphgen
out = {}
gold = os.path.join(ROOT, "tests", "golden")
for name, tag, fixedp in (("c1", "ps_fp1", 1), ("window_small", "ps", None)):
    d = dict(np.load(os.path.join(gold, name + ".npz")))
    fp = int(d["fixedp"]) if fixedp is None else fixedp
    o = HipProblem(d).raw_step("weights_pose", fp)
    out[name] = dict(dX=rel(o["dX"].reshape(-1), d[tag + ".f64.dX"].reshape(-1)),
                     poses=rel(o["poses_out"], d[tag + ".f64.poses_out"]), status=int(o["status"]))
    so = HipProblem(d).raw_step("weights", fp, True)                       # structure-only path of the same variant
    out[name]["so_patches"] = rel(so["patches_out"], d["so.f64.patches_out"])
g = graphgen.make_config("C3", seed=0)
f = lambda a: np.asarray(a, np.float32).astype(np.float64)
d = dict(poses=f(g.poses), patches=f(g.patches), mono=f(g.mono_disp), intrinsics=f(g.intrinsics), targets3=f(g.targets3),
         weights=f(g.weights), weights_pose=f(g.weights_pose), ii=g.ii, jj=g.jj, kk=g.kk, bounds=np.asarray(g.bounds, np.float64))
gd = dict(np.load(os.path.join(gold, "c3.npz")))
o = HipProblem(d).raw_step("weights_pose", 1)
out["c3"] = dict(dX=rel(o["dX"].reshape(-1), gd["ps.f64.dX"].reshape(-1)), poses=rel(o["poses_out"], gd["ps.f64.poses_out"]),
                 status=int(o["status"]))
print("RESULT " + json.dumps(out))
"""

# (environment, tolerance on dX, tolerance on the new poses).  Float64 per-edge maths and a float64 factor in LDS: dX is
# inside north_star's 1e-5 (measured 2.6e-8 — it is stored as float32).  The float variants of the solver factor in
# float32 and refine once; BT_FORCE prec=f32 is the float32 per-edge path of round 2 (the reference's own precision: its
# float32 run is 5e-3 off in dX on these fixtures).
VARIANTS = [
    ((), 1e-5, 2e-7),
    (("solver=fused",), 1e-5, 2e-7),                              # one workgroup barrier per level instead of flags
    (("solver=lds",), 1e-5, 2e-7),                                # the two-phase k_solve_lds<double>
    (("solver=lds", "order=natural"), 1e-5, 2e-7),
    (("prec=f32",), 2e-3, 1e-5),                                  # float32 per edge, 8 / 16 waves per tile as the plan picks
    (("prec=f32", "wide=1"), 2e-3, 1e-5),                         # 16-wave float32 k_tile forced
    (("prec=f32", "wide=0"), 2e-3, 1e-5),
    (("solver=lds32",), 5e-5, 1e-6),
    (("solver=global",), 5e-5, 1e-6),
]


@pytest.mark.parametrize("env,tol_dx,tol_pose", VARIANTS, ids=lambda v: (",".join(v) or "default") if isinstance(v, tuple) else None)
def test_solver_variant(env, tol_dx, tol_pose):
    import force
    e = force.env_with(*env)                      # (BT_FORCE tokens on top of whatever the suite already runs under)
    if force.f32_edges(e):
        tol_dx, tol_pose = max(tol_dx, 2e-3), max(tol_pose, 1e-5)         # float32 per-edge maths (forced by the environment)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + SCRIPT], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[7:])
    for name, v in res.items():
        assert v["status"] == 0, (name, v)
        assert v["dX"] < tol_dx and v["poses"] < tol_pose, (env, name, v)
        assert v.get("so_patches", 0.0) < 1e-5, (env, name, v)
