"""-m gpu: the per-edge mask, loss and clamp branches (batrack_amd/csrc/ba_edge.hpp: edge_eval<float>, edge_eval<double>,
edge_eval_mixed; ba_update.hpp: clamp_disp, new_disp, update_rest) through every kernel family that reaches them.

The problems are tests/mask_problems.py's (tests/test_edge_masks_cpu.py shows that the oracle decides every threshold alike in
float64 and float32 on them, with margins of 1000 float32 ulps and more): points on a camera's plane, thinly in front of it and
behind it, projections just outside and just inside each border, residuals of 249 and 251 px, the huber knee, tracks pushed
through either end of the clamp, start disparities outside it with and without a track, tracks whose every edge is masked —
mixed with ordinary tracks in the same tiles.

BT_FORCE is read once per process: one child process per variant

    ()                   k_tile, float64 per edge, k_solve_update (fused)      ("upd=split",)       k_tile + k_update
    ("prec=f32",)        k_tile, float32 per edge                              ("kernel=k_etile",)  the pair-major tile kernel
    ("kernel=k_stream",) mixed precision                                       ("kernel=k_edge2",)  k_edge2 + k_edge2u, mixed

runs every case (mask_problems.CASES: base, deep and loose, each as a pose+structure and as a structure-only step; base also
under the cauchy and the trivial loss; loose's hub tracks through k_loose_*) and leaves its outputs in a file.  Per case, against
oracle.ba_step in float64: status 0, nothing non-finite, the project's gates by the plan's edge precision (GATES of
tests/test_gpu_jacobian_kernels.py) on lower S, y, dX, the pose update over the free poses, the disparity update over the
tracks that are not clamped, and the state; bit for bit: the clamped disparities, the trackless patches, the patches outside
the graph, and the poses of a structure-only step.

"Masked means absent": every pose+structure case runs again on the same plan and workspace with the weights of the edges the
oracle masks set to 0; S, y, dX and both outputs must come out bit for bit as before.  [S | y] is accumulated by float64 atomics
of several workgroups, so two runs of the SAME inputs agree only up to the order of those adds
(test_reduced_system_is_reproducible_step_after_step: 1e-9): the unmodified case runs three times, and only where those three
agree bit for bit is the masked run held to the bits; elsewhere it is held to the route's `sys` gate on S and y, its `dx` gate
on dX and its `state` gate on the outputs, against the first run.  (Measured on the MI355X: the float64 tile routes' three
runs were 4e-17 .. 3e-15 apart in [S | y] every time, k_stream, k_edge2 and prec=f32 bit-equal in one process and not in the
next; a masked edge that leaked into one of the
pair products or per-track sums would show at 1e-3.)

Gates.  The float64 routes hold the project's gates.  The float32 and mixed routes exceed them on these inputs (disparities of
8 to 12, 249 px residuals at full weight under the trivial loss): the quantities of ORACLE_GATED are held to the larger of the
project's gate and twice the float32 ORACLE's own distance from the float64 oracle on the same problem, never to anything taken
from the kernels' output; DESIGN.md §5 records the measured figures (the closest: k_edge2 under the trivial loss, dX 1.5e-3
against the float32 oracle's 8.5e-4).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import force
import mask_problems as mp
from gpu_util import rel, update_err
from test_gpu_jacobian_kernels import GATES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import mask_problems as mp
from gpu_util import HipProblem
from batrack_amd.plan import Plan, Stepper

out = {}
for name in mp.BUILDERS:
    d, info = mp.problem(name)
    hp = HipProblem(d)
    plan = Plan(hp.ii, hp.jj, hp.kk, hp.poses.shape[1], hp.patches.shape[1], info["fixedp"])
    st = Stepper(plan, "cuda:0")
    out[name + ".kernel"] = np.asarray(plan.jacobian_kernel)
    out[name + ".prec"] = np.asarray(plan.edge_precision)
    out[name + ".n"] = np.asarray(plan.n)
    for k in ("trk_loc", "kx", "lz_trk"):
        out[name + "." + k] = plan.array(k)
    P, pat = hp.poses[0].contiguous(), hp.patches.reshape(-1, 3).contiguous()
    tg = hp.t3[0]
    D = 6 * plan.n

    def step(key, w, so, loss):
        # a whole step (the fused solve + update launch where the route has one), then the same step in its two phases for [S | y]
        Pout, pout = torch.full_like(P, float("nan")), torch.full_like(pat, float("nan"))
        args = (P, pat, hp.mono.reshape(-1), hp.intr[0], tg, tg.stride(0), w, Pout, pout, hp.bounds, 1e-4, 10.0, 0.05, loss, so)
        st.step(*args)
        torch.cuda.synchronize()
        out[key + ".poses"], out[key + ".patches"] = Pout.cpu().numpy(), pout.cpu().numpy()
        if so:
            return
        out[key + ".dX"], out[key + ".status"] = st.dx.cpu().numpy(), np.asarray(st.status())
        assert float(st.system.abs().max()) == 0.0                  # accumulators left clear
        Pout.fill_(float("nan")); pout.fill_(float("nan"))
        st.step(*args, phase="reduce")
        torch.cuda.synchronize()
        sysv = st.system.cpu().numpy().copy()
        out[key + ".S"], out[key + ".y"] = sysv[:D * D].reshape(D, D), sysv[D * D:]
        st.step(*args, phase="solve_update")
        torch.cuda.synchronize()
        out[key + ".phased.poses"], out[key + ".phased.patches"], out[key + ".phased.dX"] = Pout.cpu().numpy(), pout.cpu().numpy(), st.dx.cpu().numpy()

    for case, (prob, so, loss) in mp.CASES.items():
        if prob != name:
            continue
        w = hp.w[mp.wkey(so)][0].contiguous()
        step(case + ".0", w, so, loss)
        if not so:
            step(case + ".1", w, so, loss)
            valid = torch.as_tensor(mp.oracle_edges(case)["valid"] > 0, device=w.device)
            step(case + ".masked", (w * valid[:, None]).contiguous(), so, loss)
            step(case + ".2", w, so, loss)
np.savez(sys.argv[1], **out)
"""

VARIANTS = [(), ("upd=split",), ("prec=f32",), ("kernel=k_etile",), ("kernel=k_stream",), ("kernel=k_edge2",)]
# the kernel the base graph must take under each variant, and the one `deep` must take where the issue names it
BASE_KERNEL = {(): "k_tile", ("upd=split",): "k_tile", ("prec=f32",): "k_tile", ("kernel=k_etile",): "k_etile",
               ("kernel=k_stream",): "k_stream", ("kernel=k_edge2",): "k_edge2"}
GATE_NAMES = ("state", "sys", "dx", "upd_pose", "upd_disp")
# (edge precision, quantity) gated at twice the float32 ORACLE's own distance from the float64 oracle on the same problem instead
# of the project's gate, which these inputs (disparities of 8 to 12, points near a camera's plane) exceed: DESIGN.md has the
# measured figures
ORACLE_GATED = {(4, "sys"), (4, "dx"), (4, "upd_pose"), (6, "sys"), (6, "dx"), (6, "upd_pose"), (6, "upd_disp"), (6, "state")}


def gate_of(prec, q, gates, e32):
    """never from the kernel's output: the project's gate, or where listed the larger of it and twice the float32 oracle's distance"""
    return max(gates[q], 2 * e32[q]) if (prec, q) in ORACLE_GATED else gates[q]


_FAULTED = []
PARAMS = [pytest.param(v, c, id=(",".join(v) or "default") + "-" + c) for v in VARIANTS for c in mp.CASES]


@functools.lru_cache(maxsize=None)
def run_variant(toks):
    """The outputs of every case under these BT_FORCE tokens: one child process, started once (a failed one is cached as well)"""
    import tempfile
    if _FAULTED:
        return None, f"not started: the child process of {_FAULTED[0]} was killed or timed out"
    path = os.path.join(tempfile.mkdtemp(prefix="edge_masks_"), "out.npz")
    try:
        r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + SCRIPT, path], env=force.env_with(*toks),
                           capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _FAULTED.append(toks)
        return None, f"child process of {toks} timed out"
    if r.returncode != 0:
        if r.returncode < 0 or r.returncode > 128:                 # killed by a signal: no further process is started on the GPU
            _FAULTED.append(toks)
        return None, f"child process of {toks} ended with {r.returncode}: {r.stderr[-3000:]}"
    return dict(np.load(path)), ""


@functools.lru_cache(maxsize=None)
def reference(case, dtype=np.float64):
    return mp.reference(case, dtype)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def errors(o, ref, d, info, so, n):
    """the gated quantities of outputs o (S, y, dX, poses, patches) against ref"""
    act = np.unique(d["kk"])
    unclamped = act[(ref["patches_out"][act, 2] > mp.LO) & (ref["patches_out"][act, 2] < mp.HI)]
    e = dict(upd_disp=update_err(o["patches"][:, 2], ref["patches_out"][:, 2], d["patches"][:, 2], unclamped),
             state=rel(o["patches"], ref["patches_out"]))
    if not so:
        free = np.arange(info["fixedp"], info["fixedp"] + n)
        e.update(sys=max(rel(np.tril(o["S"]), np.tril(ref["S"])), rel(o["y"], ref["y"])), dx=rel(o["dX"].reshape(-1), ref["dX"].reshape(-1)),
                 upd_pose=update_err(o["poses"], ref["poses_out"], d["poses"], free),
                 state=max(e["state"], rel(o["poses"], ref["poses_out"])))
    return e


@pytest.mark.parametrize("toks", VARIANTS, ids=lambda v: ",".join(v) or "default")
def test_each_variant_runs_the_kernel_it_is_meant_to(toks):
    res, err = run_variant(toks)
    assert res is not None, err
    kern = {name: str(res[name + ".kernel"]) for name in mp.BUILDERS}
    assert kern["base"] == BASE_KERNEL[toks], kern
    if toks == ("kernel=k_stream",):
        assert kern["deep"] == "k_stream", kern
    if toks == ("kernel=k_etile",):
        assert kern["deep"] == "k_etile", kern                      # (the plan's jacobian_kernel names the pair-major kernel)
    for name in mp.BUILDERS:
        k, prec = kern[name], int(res[name + ".prec"])
        assert prec == (6 if k in ("k_stream", "k_edge2") else 4 if toks == ("prec=f32",) else 8), (name, k, prec)
        info = mp.problem(name)[1]
        loc, kx = res[name + ".trk_loc"], res[name + ".kx"]
        if name == "loose":
            # the hubs sit in no tile: ba_loose.hip's kernels step them (launch_loose_reduce / launch_loose_update run for lz_trk)
            assert sorted(kx[loc < 0]) == sorted(kx[res[name + ".lz_trk"]]) == sorted(info["hubs"])
        else:
            # no special track alone in a tile: every tile that holds one holds an ordinary track as well
            tile, special = loc >> 6, np.isin(kx, info["special"])
            assert (loc >= 0).all() and all((~special[tile == t]).any() for t in tile[special]), (name, tile[special])


@pytest.mark.parametrize("toks,case", PARAMS)
def test_masks_losses_and_clamps_vs_oracle(toks, case):
    res, err = run_variant(toks)
    assert res is not None, err
    name, so, loss = mp.CASES[case]
    d, info = mp.problem(name)
    ref = reference(case)
    prec, n = int(res[name + ".prec"]), int(res[name + ".n"])
    got = lambda run, what: res[f"{case}.{run}.{what}"]
    o = {k: got("0", k) for k in (("poses", "patches") if so else ("poses", "patches", "dX", "S", "y"))}
    # status 0, nothing non-finite
    if not so:
        assert int(got("0", "status")) == 0 and not ref["failed"]
    for k, v in o.items():
        assert np.isfinite(v).all(), (k, np.argwhere(~np.isfinite(v))[:5])
    # the gates: the project's by the plan's edge precision; where listed, twice the float32 oracle's own distance
    gates = dict(zip(GATE_NAMES, GATES[prec]))
    e = errors(o, ref, d, info, so, n)
    e32 = None
    if prec != 8:
        r32 = reference(case, np.float32)
        o32 = dict(poses=r32["poses_out"], patches=r32["patches_out"])
        if not so:
            o32.update(S=r32["S"], y=r32["y"], dX=r32["dX"])
        e32 = errors(o32, ref, d, info, so, n)
    for q, err_q in e.items():
        print(f"{','.join(toks) or 'default'} {case} prec {prec} {q}: {err_q:.3g} (gate {gate_of(prec, q, gates, e32):g}, project gate {gates[q]:g}"
              + (f", float32 oracle {e32[q]:.3g}" if e32 else "") + ")")
    for q, err_q in e.items():
        gate = gate_of(prec, q, gates, e32)
        assert err_q < gate, (toks, case, q, err_q, gate)
    if not so:     # the step in its two phases (never the fused launch) gives what the whole step gives, within the same gates
        ph = dict(o, poses=got("0", "phased.poses"), patches=got("0", "phased.patches"), dX=got("0", "phased.dX"))
        for q, err_q in errors(ph, ref, d, info, so, n).items():
            gate = gate_of(prec, q, gates, e32)
            assert err_q < gate, (toks, case, "phased", q, err_q, gate)
    # exact, whatever the precision
    X = o["patches"]
    for p, bound in info["clamp"].items():
        assert X[p, 2] == np.float32(bound), (p, X[p, 2], bound)
    assert same_bits(X[:, :2], d["patches"][:, :2].astype(np.float32))            # x, y of every patch copied
    outside = np.setdiff1d(np.arange(len(X)), d["kk"])                           # no track: untouched apart from the clamp
    assert set(info["start_out_trackless"]) <= set(outside)
    assert same_bits(X[outside, 2], np.clip(d["patches"][outside, 2].astype(np.float32), np.float32(1e-3), np.float32(10.0)))
    if so:
        assert same_bits(o["poses"], d["poses"].astype(np.float32))
        return
    # masked means absent
    keys = ("S", "y", "dX", "poses", "patches", "phased.dX", "phased.poses", "phased.patches")
    reproducible = all(same_bits(got("0", k), got(r, k)) for r in ("1", "2") for k in keys)
    apart = max(rel(got(r, k), got("0", k)) for r in ("1", "2") for k in ("S", "y"))
    print(f"{','.join(toks) or 'default'} {case}: three runs of the same inputs bit-equal: {reproducible} ([S | y] {apart:.3g} apart)")
    assert apart < gates["sys"]
    if reproducible:
        for k in keys:
            assert same_bits(got("masked", k), got("0", k)), (toks, case, k, rel(got("masked", k), got("0", k)))
    else:
        for k in keys:
            g = gates["sys"] if k in ("S", "y") else gates["dx"] if k.endswith("dX") else gates["state"]
            assert rel(got("masked", k), got("0", k)) < g, (toks, case, k)
