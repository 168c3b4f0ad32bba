"""-m gpu: the wave-per-tile kernels when a wave walks SEVERAL tiles, on graphs of fewer than 50 tiles.

k_edge2 / k_edge2u (ba_edge2.hip, ba_edge2u.hip) and k_stream (ba_stream.hip) give a wave (k_stream: a workgroup)
ceil(T / (CUs x waves per CU)) tiles: one, until a graph has well over a thousand.  Everything those kernels carry from one tile to
the next — pair sums kept in registers while the lanes' pairs stay, Schur sums in LDS while the cameras stay, their flushes on a
change and after 16 tiles, the geometry reload, the context and prefetch that run a tile ahead, the merge of a workgroup's waves at
the end — is taken by no small graph.  BT_FORCE wptwaves=N (ba_plan.hpp) caps the waves of those launches and nothing else, so the
graphs of tests/wpt_graphs.py (tests/test_wpt_graphs_cpu.py shows on the host plans which path each reaches under which cap) walk 48
tiles on one wave, on three, on seven.

BT_FORCE is read once per process: one child process per configuration, kernel in {k_edge2, k_stream} x wptwaves in {unset, 1, 3, 7},
one after the other; each steps every graph and leaves its outputs in a file.  Per graph and configuration, against oracle.ba_step
in float64:

    a pose+structure step (S, y, dX, both updates, the state) and a structure-only step, under the gates of
    tests/test_gpu_jacobian_kernels.py by the plan's edge precision (GATES) — for slots1, whose tracks have ONE observation, the
    gates that file's _ONE_OBS states on S, y, the poses and the patches, for the reason given there;
    plan.jacobian_kernel is the forced kernel, or what the fall-through cases take (test_wpt_graphs_cpu.KERNEL);
    five pose+structure steps of the one plan, each like the first (same_step of tests/test_gpu_shift_tables.py: rel 1e-6);
    band and slots3 with one lmbda per track (against the operator-sequence oracle, oracle/refseq.py, in float64);
    band under the cauchy and the trivial loss (k_edge2 is instantiated per loss).

The capped configurations get exactly the gates of the uncapped one.  What a capped run differs by from the uncapped run of the same
kernel is printed, not gated: float32 pair sums carried over more tiles differ in the last digits."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import force
import oracle
import wpt_graphs as wg
from gpu_util import rel, update_err
from test_gpu_jacobian_kernels import GATES
from test_wpt_graphs_cpu import KERNEL, FIGURES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (graph, loss, per-track lmbda) beside the huber / scalar-lmbda steps every graph gets
EXTRA = [("band", "cauchy", False), ("band", "trivial", False), ("band", "huber", True), ("slots3", "huber", True)]

SCRIPT = r"""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import wpt_graphs as wg
from gpu_util import HipProblem
from batrack_amd.plan import Plan, Stepper

kernel, EXTRA = sys.argv[2], eval(sys.argv[3])
out = {}
torch.zeros(1, device="cuda:0"); torch.cuda.synchronize()
gpu_s = 0.0
for name in wg.GRAPHS[kernel]:
    d, fixedp = wg.inputs(name)
    hp = HipProblem(d)
    t0 = time.perf_counter()
    plan = Plan(hp.ii, hp.jj, hp.kk, hp.poses.shape[1], hp.patches.shape[1], fixedp)
    st = Stepper(plan, "cuda:0")
    out[name + ".kernel"], out[name + ".prec"] = np.asarray(plan.jacobian_kernel), np.asarray(plan.edge_precision)
    out[name + ".n"], out[name + ".tiles"] = np.asarray(plan.n), np.asarray(plan.tiles)
    P, pat, tg = hp.poses[0].contiguous(), hp.patches.reshape(-1, 3).contiguous(), hp.t3[0]
    D = 6 * plan.n

    def step(key, so, loss="huber", lm=None, phased=True):
        w = hp.w["weights" if so else "weights_pose"][0].contiguous()
        Pout, pout = torch.full_like(P, float("nan")), torch.full_like(pat, float("nan"))
        args = (P, pat, hp.mono.reshape(-1), hp.intr[0], tg, tg.stride(0), w, Pout, pout, hp.bounds, 1e-4, 10.0, 0.05, loss, so)
        if phased and not so:       # the step split where a multi-GPU run all-reduces, so that [S | y] can be read
            st.step(*args, phase="reduce", lmbda_per_track=lm)
            torch.cuda.synchronize()
            sysv = st.system.cpu().numpy().copy()
            out[key + ".S"], out[key + ".y"] = sysv[:D * D].reshape(D, D), sysv[D * D:]
            st.step(*args, phase="solve_update", lmbda_per_track=lm)
        else:
            st.step(*args, lmbda_per_track=lm)
        torch.cuda.synchronize()
        out[key + ".poses"], out[key + ".patches"] = Pout.cpu().numpy(), pout.cpu().numpy()
        if not so:
            out[key + ".dX"], out[key + ".status"] = st.dx.cpu().numpy(), np.asarray(st.status())
            assert float(st.system.abs().max()) == 0.0              # accumulators left clear

    step(name + ".ps", False)
    step(name + ".so", True)
    for k in range(5):                                              # the whole step, five times on the one plan and workspace
        step(f"{name}.rep{k}", False, phased=False)
    for g, loss, per_track in EXTRA:
        if g == name:
            lm = torch.as_tensor(wg.lmbda_per_track(name), device="cuda:0") if per_track else None
            step(f"{name}.{loss}.{'lm' if per_track else 'ps'}", False, loss, lm)
            step(f"{name}.{loss}.{'lm' if per_track else 'ps'}.so", True, loss, lm)
    gpu_s += time.perf_counter() - t0
out["seconds"] = np.asarray(gpu_s)
np.savez(sys.argv[1], **out)
"""

CONFIGS = [(k, c) for k in ("k_edge2", "k_stream") for c in wg.CAPS]
_FAULTED = []


@functools.lru_cache(maxsize=None)
def run_config(kernel, cap):
    """The outputs of every graph under BT_FORCE kernel=..., wptwaves=cap: one child process, started once (a failed one is cached as
    well; after a child that was killed or timed out no further one is started)"""
    import tempfile
    if _FAULTED:
        return None, f"not started: the child process of {_FAULTED[0]} was killed or timed out"
    path = os.path.join(tempfile.mkdtemp(prefix="wpt_walks_"), "out.npz")
    toks = (f"kernel={kernel}",) + (() if cap is None else (f"wptwaves={cap}",))
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + SCRIPT, path, kernel, repr(EXTRA)], env=force.env_with(*toks),
                           capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _FAULTED.append(toks)
        return None, f"child process of {toks} timed out"
    if r.returncode != 0:
        if r.returncode < 0 or r.returncode > 128:
            _FAULTED.append(toks)
        return None, f"child process of {toks} ended with {r.returncode}: {r.stderr[-3000:]}"
    res = dict(np.load(path))
    print(f"child {','.join(toks)}: {time.perf_counter() - t0:.1f} s in all, {float(res['seconds']):.2f} s planning and stepping the graphs")
    return res, ""


@functools.lru_cache(maxsize=None)
def reference(name, so, loss="huber", per_track=False):
    d, fixedp = wg.inputs(name)
    w = d["weights" if so else "weights_pose"]
    if not per_track:
        return oracle.ba_step(d["poses"], d["patches"], d["mono"], d["intrinsics"], d["targets3"], w, d["ii"], d["jj"], d["kk"], d["bounds"],
                              fixedp=fixedp, structure_only=so, loss=loss, want_system=not so)
    import torch
    from oracle import refseq
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    lm = wg.lmbda_per_track(name)                           # float32 values, as the step receives them
    r = refseq.ba_step(t(d["poses"]), t(d["patches"]), t(d["mono"]), t(d["intrinsics"]), t(d["targets3"]), t(w), torch.as_tensor(d["ii"]),
                       torch.as_tensor(d["jj"]), torch.as_tensor(d["kk"]), [float(x) for x in d["bounds"]], fixedp=fixedp, structure_only=so,
                       loss=loss, lmbda=t(lm), want_system=not so)
    return {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in r.items()}


def errors(res, key, ref, d, fixedp, so, n):
    """-> {quantity: error against the reference}: sys (lower S and y, the larger), dx, upd_pose, upd_disp, state; and the four figures
    of the one-observation gates"""
    act = np.unique(d["kk"])
    X = res[key + ".patches"]
    e = dict(upd_disp=update_err(X[:, 2], ref["patches_out"][:, 2], d["patches"][:, 2], act), state=rel(X, ref["patches_out"]))
    e["patches"] = e["state"]
    if not so:
        P = res[key + ".poses"]
        e.update(S=rel(np.tril(res[key + ".S"]), np.tril(ref["S"])), y=rel(res[key + ".y"], ref["y"]),
                 dx=rel(res[key + ".dX"].reshape(-1), np.asarray(ref["dX"]).reshape(-1)),
                 upd_pose=update_err(P, ref["poses_out"], d["poses"], np.arange(fixedp, fixedp + n)), poses=rel(P, ref["poses_out"]))
        e["sys"] = max(e["S"], e["y"])
        e["state"] = max(e["state"], e["poses"])
    return e


def gates_for(name, prec, so):
    """{quantity: gate}: GATES by the plan's edge precision; the one-observation graph under the mixed kernels: _ONE_OBS's"""
    if name == "slots1" and prec == 6 and not so:
        return dict(S=5e-6, y=1e-4, poses=3e-4, patches=5e-6)
    g = dict(zip(("state", "sys", "dx", "upd_pose", "upd_disp"), GATES[prec]))
    return {k: g[k] for k in (("state", "upd_disp") if so else g)}


def check(res, label, key, name, so, loss="huber", per_track=False):
    d, fixedp = wg.inputs(name)
    ref = reference(name, so, loss, per_track)
    prec, n = int(res[name + ".prec"]), int(res[name + ".n"])
    for k in ("poses", "patches") + (() if so else ("S", "y", "dX")):
        assert np.isfinite(res[f"{key}.{k}"]).all(), (label, key, k)
    if so:
        assert res[key + ".poses"].tobytes() == d["poses"].astype(np.float32).tobytes()      # a structure-only step copies the poses
    else:
        assert int(res[key + ".status"]) == 0 and not ref["failed"]
    e, gates = errors(res, key, ref, d, fixedp, so, n), gates_for(name, prec, so)
    print(f"{label} {key} prec {prec}: " + ", ".join(f"{q} {e[q]:.3g} (gate {g:g})" for q, g in gates.items()))
    for q, g in gates.items():
        assert e[q] < g, (label, key, q, e[q], g)


PARAMS = [pytest.param(k, c, n, id=f"{k}-{'uncapped' if c is None else 'wptwaves' + str(c)}-{n}") for k, c in CONFIGS for n in wg.GRAPHS[k]]


@pytest.mark.parametrize("kernel,cap,name", PARAMS)
def test_steps_of_every_graph_vs_oracle(kernel, cap, name):
    res, err = run_config(kernel, cap)
    assert res is not None, err
    label = f"{kernel} cap {cap}"
    # the kernel the table says, on the tiles the CPU test pins
    assert str(res[name + ".kernel"]) == KERNEL[kernel][name], (label, name, str(res[name + ".kernel"]))
    assert int(res[name + ".prec"]) == (6 if KERNEL[kernel][name] in ("k_edge2", "k_stream") else 8)
    if KERNEL[kernel][name] == kernel:
        assert int(res[name + ".tiles"]) == FIGURES[kernel][name][0]
    check(res, label, name + ".ps", name, False)
    check(res, label, name + ".so", name, True)
    for g, loss, per_track in EXTRA:
        if g == name:
            key = f"{name}.{loss}.{'lm' if per_track else 'ps'}"
            check(res, label, key, name, False, loss, per_track)
            check(res, label, key + ".so", name, True, loss, per_track)
    if any(g == name and pt for g, _, pt in EXTRA):         # ... and the per-track values are not the scalar's result
        assert rel(res[f"{name}.huber.lm.patches"][:, 2], res[f"{name}.ps.patches"][:, 2]) > 1e-4
    # five steps of the one plan: each like the first (same_step, tests/test_gpu_shift_tables.py)
    from test_gpu_shift_tables import same_step
    d, _ = wg.inputs(name)
    first = (res[name + ".rep0.poses"], res[name + ".rep0.patches"], int(res[name + ".rep0.status"]), d["poses"])
    for k in range(1, 5):
        same_step((res[f"{name}.rep{k}.poses"], res[f"{name}.rep{k}.patches"], int(res[f"{name}.rep{k}.status"]), d["poses"]), first)
    if cap is not None:                                     # printed, not gated (see the top)
        base, err = run_config(kernel, None)
        assert base is not None, err
        print(f"{label} {name} against uncapped: " + ", ".join(f"{q} {rel(res[f'{name}.ps.{q}'], base[f'{name}.ps.{q}']):.3g}" for q in ("S", "y", "dX")))
