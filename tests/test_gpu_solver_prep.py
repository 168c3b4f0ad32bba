"""-m gpu: the LDS solvers' back-substitution preparation (ba_solve.hip: lds_backsub_prep, one thread per factor block) and their
load, at the smallest shapes at which they can go wrong:

  one      one free pose: a diagonal block only — no thread has a panel, zt must still be formed
  two      two free poses: one off-diagonal block
  chain    graphgen.make_graph(12, 16, 8): a two-ended chain with a separator at its smallest
  blocks   the smallest make_graph(n, 8, 8) whose factor has more blocks than the solver has threads (768), so that the block
           loop takes a second round: n = 74, 776 blocks, a float32 factor (k_solve_lds<float>) — both facts asserted from the plan
  retry    the c1 fixture with a NaN put into y: the factorisation succeeds, dX is NaN, the second attempt (stronger damping)
           runs the load and the preparation again and cannot cure it (status 2); the untouched system then solves as before

under the default solver and with each LDS solver forced.  dX and the new poses against oracle.ba_step in float64 at the
tolerances of tests/test_gpu_solver_variants.py; the status is 0 (2 after the NaN); two consecutive steps from the same inputs
give the same dX bit for bit (nothing the solver leaves behind in the workspace may reach the next step): whole steps where
the factor is float64, and in every case one reduced system [S | y] solved twice, which takes the reduction's atomics out.

Known to miss on "blocks": k_solve_lds<float> updates the destinations that several columns of a level share with LDS atomics,
whose order varies from run to run, and neither the parent commit nor this one repeats bit for bit there.  Measured on the
MI355X, one reduced system solved five times, largest difference of dX (|dX| <= 0.037): parent commit 0 on this graph and
1.8e-12 on make_graph(60, 8, 8), this commit 1.5e-11 and 0; five whole steps: parent 3.6e-12 and 0, this commit 9.1e-13 and
1.8e-12 — the last bit of dX's small entries, in some runs and not in others.  The sweep is not part of this change.

BT_FORCE is read once per process, so each environment runs one child process, which takes all of its cases."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVER_THREADS = 768                     # ba_kernels.hpp: kSolveThreads
GRAPHS = {"one": (2, 16, 8), "two": (3, 16, 8), "chain": (12, 16, 8), "blocks": (74, 8, 8)}

SCRIPT = r"""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
from gpu_util import HipProblem
from batrack_amd import graphgen
from batrack_amd.plan import Plan, Stepper

def inputs(name):
    if name == "retry":
        return dict(np.load(os.path.join(ROOT, "tests", "golden", "c1.npz")))
    g = graphgen.make_graph(*GRAPHS[name])
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return dict(poses=f(g.poses), patches=f(g.patches), mono=f(g.mono_disp), intrinsics=f(g.intrinsics), targets3=f(g.targets3),
                weights=f(g.weights), weights_pose=f(g.weights_pose), ii=g.ii, jj=g.jj, kk=g.kk, bounds=np.asarray(g.bounds, np.float64))

out = {}
for name in CASES:
    hp = HipProblem(inputs(name))
    plan = Plan(hp.ii, hp.jj, hp.kk, hp.poses.shape[1], hp.patches.shape[1], 1)
    st = Stepper(plan, "cuda:0")
    P, pat = hp.poses[0].contiguous(), hp.patches.reshape(-1, 3).contiguous()
    Pout, pout = torch.empty_like(P), torch.empty_like(pat)
    tg = hp.t3[0]
    args = (P, pat, hp.mono.reshape(-1), hp.intr[0], tg, tg.stride(0), hp.w["weights_pose"][0].contiguous(),
            Pout, pout, hp.bounds, 1e-4, 10.0, 0.05, "huber", False)
    r = dict(n=int(plan.n), nnzb=int(plan.nnz_blocks), solver_mode=int(plan.solver_mode), status=[])
    st.step(*args)
    torch.cuda.synchronize()
    r["status"].append(int(st.status()))
    dx1 = st.dx.clone()
    r["dX"] = dx1.cpu().numpy().astype(np.float64).reshape(-1).tolist()
    r["poses"] = Pout.cpu().numpy().astype(np.float64).reshape(-1).tolist()
    D = 6 * plan.n
    st.step(*args, phase="reduce")                         # one reduced system [S | y], kept: a solve clears it
    good = st.system.clone()
    if name == "retry":
        st.system[D * D + 3] = float("nan")
        st.step(*args, phase="solve_update")
        torch.cuda.synchronize()
        r["status"].append(int(st.status()))
        r["nan_dx"] = bool(torch.isnan(st.dx).any())
        st.system.copy_(good)
    st.step(*args, phase="solve_update")
    torch.cuda.synchronize()
    r["status"].append(int(st.status()))
    dx2, P2 = st.dx.clone(), Pout.clone()
    st.system.copy_(good)
    st.step(*args, phase="solve_update")
    torch.cuda.synchronize()
    r["status"].append(int(st.status()))
    # (a) two whole steps from the same inputs, (b) the same reduced system solved twice: without the reduction's atomics
    r["same_step"] = bool(torch.equal(dx2, dx1))
    r["step_apart"] = float((dx2 - dx1).abs().max())
    r["same_solve"] = bool(torch.equal(st.dx, dx2) and torch.equal(Pout, P2))
    r["solve_apart"] = float((st.dx - dx2).abs().max())
    r["dx_max"] = float(dx1.abs().max())
    out[name] = r
print("RESULT " + json.dumps(out))
"""

# (BT_FORCE tokens, the cases of that process, tolerance on dX, tolerance on the new poses): the float64 factors inside
# north_star's 1e-5, the float32 factor with its refinement at the gates tests/test_gpu_solver_variants.py holds it to
ENVS = [
    ((), ("one", "two", "chain", "blocks", "retry"), 1e-5, 2e-7),
    (("solver=fused",), ("one", "two", "chain", "retry"), 1e-5, 2e-7),
    (("solver=lds",), ("one", "two", "chain", "retry"), 1e-5, 2e-7),
    (("solver=lds", "order=natural"), ("one", "two", "chain"), 1e-5, 2e-7),       # levels of one column
    (("solver=lds32",), ("one", "two", "chain", "retry"), 5e-5, 1e-6),
]
PARAMS = [pytest.param(env, case, tol_dx, tol_pose, id=(",".join(env) or "default") + "-" + case)
          for env, cases, tol_dx, tol_pose in ENVS for case in cases]


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@functools.lru_cache(maxsize=None)
def run_env(env):
    import force
    cases = next(c for e, c, _, _ in ENVS if e == env)
    e = force.env_with(*env)
    head = f"ROOT = {ROOT!r}\nGRAPHS = {GRAPHS!r}\nCASES = {cases!r}\n"
    r = subprocess.run([sys.executable, "-c", head + SCRIPT], env=e, capture_output=True, text=True, timeout=600)
    # (a failed child is cached like a good one: a process that faulted on the GPU is started once, not once per case)
    if r.returncode != 0:
        return None, f"child process of {env} ended with {r.returncode}: {r.stderr[-2000:]}"
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:]), force.f32_edges(e)


@functools.lru_cache(maxsize=None)
def reference(case):
    """dX and the new poses of the float64 oracle, once per graph."""
    if case == "retry":
        d = dict(np.load(os.path.join(ROOT, "tests", "golden", "c1.npz")))
        return d["ps_fp1.f64.dX"], d["ps_fp1.f64.poses_out"]
    import oracle
    from batrack_amd import graphgen
    g = graphgen.make_graph(*GRAPHS[case])
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    ref = oracle.ba_step(f(g.poses), f(g.patches), f(g.mono_disp), f(g.intrinsics), f(g.targets3), f(g.weights_pose),
                         g.ii, g.jj, g.kk, g.bounds, fixedp=1, want_system=True)
    return ref["dX"], ref["poses_out"]


@pytest.mark.parametrize("env,case,tol_dx,tol_pose", PARAMS)
def test_solver_prep(env, case, tol_dx, tol_pose):
    res, f32_edges = run_env(env)
    assert res is not None, f32_edges
    v = res[case]
    import force
    forced = force.tokens(force.env_with(*env)).get("solver")         # (this case's tokens on top of what the suite runs under)
    if case == "blocks":
        # more factor blocks than threads, and still the LDS-resident float32 factor: k_solve_lds<float> (solver_mode 1)
        assert v["nnzb"] > SOLVER_THREADS and v["solver_mode"] == 1, (v["nnzb"], v["solver_mode"])
        tol_dx, tol_pose = 5e-5, 1e-6
    elif forced in ("lds32", "global"):
        assert v["solver_mode"] == (1 if forced == "lds32" else 2), v["solver_mode"]
    else:
        assert v["solver_mode"] == 0, v["solver_mode"]               # the float64 factor in LDS: k_solve_pipe / _fused / _lds<double>
    if case == "one":
        assert v["n"] == 1 and v["nnzb"] == 1, (v["n"], v["nnzb"])
    if case == "two":
        assert v["n"] == 2 and v["nnzb"] == 3, (v["n"], v["nnzb"])
    if f32_edges:
        tol_dx, tol_pose = max(tol_dx, 2e-3), max(tol_pose, 1e-5)         # float32 per-edge maths (forced by the environment)
    dX, poses = reference(case)
    e_dx, e_pose = rel(v["dX"], dX), rel(v["poses"], poses)
    print(f"{env} {case}: n {v['n']} blocks {v['nnzb']} solver_mode {v['solver_mode']} status {v['status']} "
          f"dX {e_dx:.3g} (gate {tol_dx:g}) poses {e_pose:.3g} (gate {tol_pose:g})")
    print(f"   two steps: dX {v['step_apart']:.3g} apart; one reduced system solved twice: {v['solve_apart']:.3g} apart (|dX| <= {v['dx_max']:.3g})")
    if case == "retry":
        assert v["status"] == [0, 2, 0, 0] and v["nan_dx"], v["status"]
    else:
        assert v["status"] == [0, 0, 0], v["status"]
    assert e_dx < tol_dx and e_pose < tol_pose, (env, case, e_dx, e_pose)
    # equal, bit for bit.  Whole steps with the float64 factor; with the float32 factor the one reduced system solved twice
    # ([S | y] itself is summed by atomics whose order varies: the same graph reduced three times gave S up to 5.6e-9 apart,
    # which a float64 factor's float32 dX does not show and a float32 factor's does).
    assert v["same_solve"], (env, case, v["solve_apart"])
    if v["solver_mode"] == 0:
        assert v["same_step"], (env, case, v["step_apart"])
