"""-m gpu: the fused solve + update launch (k_solve_update, batrack_amd/csrc/ba_solve_update.hpp) gives the bits of the two
launches it replaces.

On the k_tile routes with a double LDS solver a pose+structure step runs the reduced solver and the step's last kernel in one
launch: the solver's workgroup publishes dX as tagged granules, the update workgroups behind it have done everything that
does not need dX by then.  BT_FORCE upd=split launches k_solve_* and k_update apart, as before; the arithmetic is the same
expressions in the same order, so poses and patches must be EQUAL, and so must the status word.  BT_FORCE is read once per
process: every variant is one child process that runs all the cases and leaves their outputs in a file; the tests compare."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
from gpu_util import HipProblem
from batrack_amd import graphgen
from batrack_amd.plan import Plan, Stepper

out = {}
f = lambda a: np.asarray(a, np.float32).astype(np.float64)


def as_dict(g, keep=None):
    d = dict(poses=f(g.poses), patches=f(g.patches), mono=f(g.mono_disp), intrinsics=f(g.intrinsics), targets3=f(g.targets3),
             weights=f(g.weights), weights_pose=f(g.weights_pose), ii=g.ii, jj=g.jj, kk=g.kk, bounds=np.asarray(g.bounds, np.float64))
    if keep is not None:
        for k in ("targets3", "weights", "weights_pose", "ii", "jj", "kk"):
            d[k] = d[k][keep]
    return d


def run(name, d, fixedp, steps=1, timed=True, **kw):
    # `steps` whole steps (bt_ba_step) on ONE workspace, each from the poses and patches the one before left (ping-pong)
    hp = HipProblem(d)
    plan = Plan(hp.ii, hp.jj, hp.kk, hp.poses.shape[1], hp.patches.shape[1], fixedp)
    st = Stepper(plan, "cuda:0")
    P = [hp.poses[0].clone(), torch.empty_like(hp.poses[0])]
    X = [hp.patches.reshape(-1, 3).clone(), torch.empty_like(hp.patches.reshape(-1, 3))]
    tg = hp.t3[0]
    lm, ep, loss = kw.get("lmbda", 1e-4), kw.get("ep", 10.0), kw.get("loss", "huber")
    args = lambda s: (P[s & 1], X[s & 1], hp.mono.reshape(-1), hp.intr[0], tg, tg.stride(0), hp.w["weights_pose"][0].contiguous(),
                      P[1 - (s & 1)], X[1 - (s & 1)], hp.bounds, lm, ep, 0.05, loss, False)
    out[name + ".tiles"] = np.asarray(plan.info["tiles"])
    out[name + ".n"] = np.asarray(plan.n)
    for s in range(steps):
        st.step(*args(s))
        torch.cuda.synchronize()
        out[f"{name}.{s}.poses"] = P[1 - (s & 1)].cpu().numpy()
        out[f"{name}.{s}.patches"] = X[1 - (s & 1)].cpu().numpy()
        out[f"{name}.{s}.dx"] = st.dx.cpu().numpy()
        out[f"{name}.{s}.status"] = np.asarray(st.status())
        assert float(st.system.abs().max()) == 0.0            # [S | y] left clear
    if timed:                                                # which kernels a timed step launches (0: not launched)
        P[0].copy_(hp.poses[0]); X[0].copy_(hp.patches.reshape(-1, 3))      # (the first step's inputs again)
        ms = st.step_timed(*args(0))
        torch.cuda.synchronize()
        out[name + ".ran"] = np.asarray([ms[k] > 0 for k in ("tile", "pair_finalize", "solve", "update")])
        out[name + ".timed.poses"] = P[1].cpu().numpy()
        so = list(args(0)); so[7] = P[0]; so[14] = True        # a structure-only step of the same plan
        ms = st.step_timed(*so)
        out[name + ".ran_so"] = np.asarray([ms[k] > 0 for k in ("tile", "pair_finalize", "solve", "update")])


# one tile, two free poses: the tracks of frame 1, seen from frames 0, 1, 2
g = graphgen.make_graph(3, 40, 3, seed=3)
run("one_tile", as_dict(g, keep=np.flatnonzero(g.ii == 1)), 1)
# 8 tiles of 64 tracks, three steps in a row on one workspace
run("eight_tiles", as_dict(graphgen.make_graph(8, 64, 5, seed=4)), 1, steps=3)
# a patch buffer with trackless patches, a pose buffer longer than the free poses, two fixed poses
run("buffers", as_dict(graphgen.make_graph(6, 48, 3, seed=5, n_buf=11)), 2)
# the solver's edge cases (tests/test_gpu_parity.py): a failed factorisation (dX = 0), and a NaN target under the huber loss,
# whose NaN in y takes the retry
d = dict(np.load(os.path.join(ROOT, "tests", "golden", "c1.npz")))
run("chol_failed", d, 1, ep=-1e9)
t = d["targets3"].copy()
t[int(np.flatnonzero(d["weights_pose"][:, 0] > 0)[5]), 0] = np.nan
run("nan_retry", dict(d, targets3=t), 1)
np.savez(sys.argv[1], **out)
"""

_RUNS = {}


def variant(tmp_path_factory, *toks):
    """The outputs of every case under these BT_FORCE tokens (one child process per variant, run once)."""
    if toks not in _RUNS:
        import force
        path = str(tmp_path_factory.mktemp("su") / "out.npz")
        r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + SCRIPT, path], env=force.env_with(*toks),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        _RUNS[toks] = dict(np.load(path))
    return _RUNS[toks]


def same_bits(a, b):
    """Equal bit for bit, and NaN exactly where the other has NaN.  (The sign of a NaN is not compared: with a NaN target the
    tiles' atomic adds into y meet NaNs of both signs in an order that changes from launch to launch: the solver's dX, the
    same kernel code on the same inputs, came out with other NaN signs in one run of this case than in the next.)"""
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and a[~na].tobytes() == b[~nb].tobytes()


def check_case(fused, split, name, steps=1, status=0):
    for s in range(steps):
        for what in ("poses", "patches", "dx"):
            assert same_bits(fused[f"{name}.{s}.{what}"], split[f"{name}.{s}.{what}"]), (name, s, what)
        assert int(fused[f"{name}.{s}.status"]) == status and int(split[f"{name}.{s}.status"]) == status, (name, s)


def check_ran(fused, split, name):
    # timed step: the fused launch is recorded under the solver's event pair, the update's entry stays 0
    assert fused[name + ".ran"].tolist() == [True, True, True, False], fused[name + ".ran"]
    assert split[name + ".ran"].tolist() == [True, True, True, True], split[name + ".ran"]
    assert same_bits(fused[name + ".timed.poses"], split[name + ".0.poses"])
    # a structure-only step launches what it launched before (timed: k_tile and k_update, no solver)
    assert fused[name + ".ran_so"].tolist() == split[name + ".ran_so"].tolist() == [True, False, False, True]


def test_one_tile_two_free_poses(tmp_path_factory):
    fused, split = variant(tmp_path_factory), variant(tmp_path_factory, "upd=split")
    assert int(fused["one_tile.tiles"]) == 1 and int(fused["one_tile.n"]) == 2
    check_case(fused, split, "one_tile")
    check_ran(fused, split, "one_tile")


def test_several_tiles_per_workgroup(tmp_path_factory):
    """updwg=3: eight tiles, the patches, the poses and the clearing of [S | y] on three update workgroups."""
    capped, split = variant(tmp_path_factory, "updwg=3"), variant(tmp_path_factory, "upd=split")
    assert int(capped["eight_tiles.tiles"]) == 8
    check_case(capped, split, "eight_tiles", steps=3)
    check_ran(capped, split, "eight_tiles")
    check_case(capped, split, "buffers")


def test_three_steps_on_one_workspace(tmp_path_factory):
    """A granule of step k must not be taken for step k + 1's: compared after every step."""
    fused, split = variant(tmp_path_factory), variant(tmp_path_factory, "upd=split")
    check_case(fused, split, "eight_tiles", steps=3)
    assert not same_bits(fused["eight_tiles.0.dx"], fused["eight_tiles.1.dx"])


def test_trackless_patches_long_pose_buffer_two_fixed_poses(tmp_path_factory):
    fused, split = variant(tmp_path_factory), variant(tmp_path_factory, "upd=split")
    assert int(fused["buffers.n"]) == 4
    check_case(fused, split, "buffers")
    check_ran(fused, split, "buffers")


def test_failed_factorisation_and_nan_retry(tmp_path_factory):
    fused, split = variant(tmp_path_factory), variant(tmp_path_factory, "upd=split")
    check_case(fused, split, "chol_failed", status=1)                  # BT_SOLVE_CHOL_FAILED
    assert np.all(fused["chol_failed.0.dx"] == 0)
    check_case(fused, split, "nan_retry", status=2)                    # BT_SOLVE_RETRIED
    assert np.isnan(fused["nan_retry.0.dx"]).any() and np.isnan(fused["nan_retry.0.poses"]).any()
    for name in ("chol_failed", "nan_retry"):                          # (and the fused run did take the fused route)
        check_ran(fused, split, name)


def test_float32_per_edge_maths(tmp_path_factory):
    """BT_FORCE prec=f32: the float instantiations of the fused kernel against k_update<false, 512, float>."""
    fused, split = variant(tmp_path_factory, "prec=f32"), variant(tmp_path_factory, "prec=f32", "upd=split")
    for name, steps in (("one_tile", 1), ("eight_tiles", 3), ("buffers", 1)):
        check_case(fused, split, name, steps=steps)
        check_ran(fused, split, name)


def test_route_that_is_not_admitted_launches_the_update_apart(tmp_path_factory):
    """The float32 LDS solver (refined in further launches) keeps solver and k_update apart; so does every structure-only step."""
    lds32 = variant(tmp_path_factory, "solver=lds32")
    for name in ("one_tile", "eight_tiles", "buffers"):
        assert lds32[name + ".ran"].tolist() == [True, True, True, True], (name, lds32[name + ".ran"])
        assert lds32[name + ".ran_so"].tolist() == [True, False, False, True]
        assert int(lds32[name + ".0.status"]) == 0
