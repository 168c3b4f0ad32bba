"""-m gpu: a workspace that starts dirty.  include/batrack_ba.h lets a caller allocate a workspace, call bt_ba_workspace_init on it and
step; a reused hipMalloc or a torch.empty from the caching allocator holds anything.  Every other test steps from torch.zeros, so here
the workspace is filled with a poison pattern first — 0xFF bytes (NaN doubles and floats, -1 ints), the word 0x3F800000 (1.0f: finite
garbage that only a comparison with the reference catches), or another plan's leftovers (a different fixture stepped in the same
buffer, the last step a failed factorisation) — then bound to a Stepper and initialised, on every Jacobian-kernel and solver path:
  (a) right after init, bt_ba_status and bt_ba_xchg_status read 0
  (b) step 1 against the float64 reference at the gates the other tests use for that path (gpu_util.TOL, the solver VARIANTS)
  (c) step 1 against the same plan stepped from a torch.zeros workspace: [S | y] within the fp64 atomics' 1e-9, the same status,
      dX within DX_SAME and the state within STATE_SAME (below)
  (d) steps 2 and 3 (a bt_ba_step) on the same inputs agree with step 1 in the same way
  (e) after every completed step [sys, sys + zero_bytes) is zero, and so are the status block's flags (refinement, dense solver)
  (f) a reduce without its solve_update, bt_ba_workspace_init, a full step: the reference's result
and, through the fused, two-phase LDS, float LDS and global solvers, the failure semantics of ba.py:9-13 and :324-325 (the dense
solver's are in test_gpu_parity).  BT_FORCE is read once per process: one child interpreter per configuration, one at a time
(the GPU is open in this process and one child)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import torch
import oracle
import force
from gpu_util import DEV, TOL, HipProblem, rel
from edge_problems import band_120_problem, hub_graph
from test_gpu_solver_variants import VARIANTS
from batrack_amd import _lib, graphgen
from batrack_amd.plan import Plan, Stepper, _raw_stream

CASES, FAILURE, DX_SAME, STATE_SAME = json.loads(sys.argv[1])
L = _lib.lib()
toks = force.tokens()
f32e = force.f32_edges()
env_key = tuple(sorted(f"{k}={v}" for k, v in toks.items()))
VGATES = {tuple(sorted(e)): (dx, p) for e, dx, p in VARIANTS}


def gates(name, mode):
    # (dX, poses) against the reference: the solver variants' gates (raised for float32 per-edge maths like their test does), the
    # forced float LDS / global solver's for the band that takes one of them by itself; gpu_util.TOL elsewhere
    key = ("solver=lds32",) if (name == "band120" and mode == 1) else ("solver=global",) if name == "band120" else env_key
    if key not in VGATES:
        return TOL["dx"], TOL["state"]
    dx, p = VGATES[key]
    return (max(dx, 2e-3), max(p, 1e-5)) if f32e else (dx, p)


GOLD = os.path.join(ROOT, "tests", "golden")
f64 = lambda a: np.asarray(a, np.float32).astype(np.float64)


def generated(d, fixedp=1, so=False):
    r = oracle.ba_step(d["poses"], d["patches"], d["mono"], d["intrinsics"], d["targets3"], d["weights_pose"], d["ii"], d["jj"], d["kk"],
                       d["bounds"], fixedp=fixedp, want_system=True)
    c = dict(d=d, fixedp=fixedp, dX=r["dX"], poses=r["poses_out"], disp=r["patches_out"][:, 2])
    if so:
        c["so_disp"] = oracle.ba_step(d["poses"], d["patches"], d["mono"], d["intrinsics"], d["targets3"], d["weights"], d["ii"], d["jj"], d["kk"],
                                      d["bounds"], fixedp=fixedp, structure_only=True)["patches_out"][:, 2]
    return c


def from_graph(g):
    return dict(poses=f64(g.poses), patches=f64(g.patches), mono=f64(g.mono_disp), intrinsics=f64(g.intrinsics), targets3=f64(g.targets3),
                weights=f64(g.weights), weights_pose=f64(g.weights_pose), ii=g.ii, jj=g.jj, kk=g.kk, bounds=np.asarray(g.bounds, np.float64))


def load(name):
    # -> inputs, fixedp, the float64 reference of the pose+structure step (dX, poses, disparities) and of the structure-only step
    if name in ("c1", "window_small"):
        d = dict(np.load(os.path.join(GOLD, name + ".npz")))
        tag, fp = ("ps_fp1", 1) if name == "c1" else ("ps", int(d["fixedp"]))
        return dict(d=d, fixedp=fp, dX=d[tag + ".f64.dX"], poses=d[tag + ".f64.poses_out"], disp=d[tag + ".f64.patches_out"][:, 2],
                    so_disp=d["so.f64.patches_out"][:, 2])
    if name == "c3":
        gd = dict(np.load(os.path.join(GOLD, "c3.npz")))
        return dict(d=from_graph(graphgen.make_config("C3", seed=0)), fixedp=1, dX=gd["ps.f64.dX"], poses=gd["ps.f64.poses_out"],
                    disp=gd["ps.f64.disp_out"])       # (its structure-only golden follows the pose+structure step: not these inputs)
    if name == "g16":                             # slot-uniform tiles: takes a forced k_edge2 / k_stream / k_etile itself
        return generated(from_graph(graphgen.make_graph(16, 64, 8, seed=1)), so=True)
    if name in ("band120", "filled120"):
        return generated(band_120_problem(filled=name == "filled120"))
    if name == "band300":
        g = graphgen.make_graph(300, 16, 6, seed=21)
        return generated(from_graph(g))
    if name == "hubs3":
        d, hubs = hub_graph(3)
        c = generated(d)
        c["hubs"] = hubs
        return c
    raise KeyError(name)


class Run:
    # one plan's steps on one problem, in a workspace of the caller's
    def __init__(self, hp, plan, ws=None):
        self.hp, self.plan = hp, plan
        self.st = Stepper(plan, DEV, ws=ws)
        assert ws is None or self.st.ws.data_ptr() == ws.data_ptr()
        self.P = hp.poses[0].contiguous()
        self.pat = hp.patches.reshape(-1, 3).contiguous()
        self.Pout, self.pout = torch.empty_like(self.P), torch.empty_like(self.pat)
        self.lay = plan.ws_layout

    def args(self, so=False, ep=10.0):
        hp, tg = self.hp, self.hp.t3[0]
        return (self.P, self.pat, hp.mono.reshape(-1), hp.intr[0], tg, tg.stride(0), hp.w["weights" if so else "weights_pose"][0].contiguous(),
                self.P if so else self.Pout, self.pout, hp.bounds, 1e-4, ep, 0.05, "huber", so)

    def init(self):
        _lib.check(L.bt_ba_workspace_init(self.plan.handle, self.st.ws.data_ptr(), _raw_stream(self.st.device)), "bt_ba_workspace_init")

    def xchg_status(self):
        s = ctypes.c_int32(-1)
        _lib.check(L.bt_ba_xchg_status(self.plan.handle, self.st.ws.data_ptr(), _raw_stream(self.st.device), ctypes.byref(s)), "bt_ba_xchg_status")
        return s.value

    def step(self, split=True, so=False):
        a = self.args(so)
        out = {}
        if split:                                 # the step in its two halves, so that [S | y] can be read in between
            self.st.step(*a, phase="reduce")
            torch.cuda.synchronize()
            out["sys"] = self.st.system.cpu().numpy().copy()
            self.st.step(*a, phase="solve_update")
        else:
            self.st.step(*a)
        torch.cuda.synchronize()
        out.update(poses=self.Pout.cpu().numpy().astype(np.float64), patches=self.pout.cpu().numpy().astype(np.float64),
                   dX=self.st.dx.cpu().numpy().astype(np.float64), status=self.st.status())
        return out

    def dirt(self):
        # (e): what a completed step must leave behind — the accumulators zero, the exchange word and the solvers' flags 0
        lay, ws = self.lay, self.st.ws
        acc = int(torch.count_nonzero(ws[lay["sys"]:lay["sys"] + lay["zero_bytes"]]))
        words = ws[lay["status"]:lay["status"] + 1024].view(torch.int32)[[1, 200, 201, 210]].cpu().tolist()
        return acc, words


fails, meas = [], {}


def expect(ok, what):
    if not ok:
        fails.append(what)


def vs_ref(o, c, tag, so=False):
    tol_dx, tol_pose = c["gates"]
    # (b) against the float64 reference
    if so:
        e = rel(o["patches"][:, 2], c["so_disp"])
        expect(e < 1e-5, f"{tag}: structure-only disparities {e:.3g} from the reference")
        return dict(so_disp=e)
    r = dict(dX=rel(o["dX"].reshape(-1), np.asarray(c["dX"]).reshape(-1)), poses=rel(o["poses"], c["poses"]),
             disp=rel(o["patches"][:, 2], c["disp"]), status=o["status"])
    expect(o["status"] == 0, f"{tag}: solver status {o['status']}")
    expect(r["dX"] < tol_dx and r["poses"] < tol_pose and r["disp"] < TOL["state"],
           f"{tag}: dX {r['dX']:.3g} (gate {tol_dx:g}), poses {r['poses']:.3g} (gate {tol_pose:g}), disparities {r['disp']:.3g} (gate {TOL['state']:g}) from the reference")
    return r


def vs_run(o, b, tag):
    # (c), (d): two steps of the same inputs — [S | y] up to the order of the fp64 atomics, the same status, dX and state alike
    r = dict(dX=rel(o["dX"], b["dX"]), state=max(rel(o["poses"], b["poses"]), rel(o["patches"], b["patches"])))
    if "sys" in o and "sys" in b:
        r["sys"] = rel(o["sys"], b["sys"])
        expect(r["sys"] <= 1e-9, f"{tag}: [S | y] {r['sys']:.3g} apart")
    expect(o["status"] == b["status"], f"{tag}: status {o['status']} != {b['status']}")
    expect(r["dX"] <= DX_SAME and r["state"] <= STATE_SAME, f"{tag}: dX {r['dX']:.3g}, state {r['state']:.3g} apart")
    return r


def check_dirt(run, tag):
    acc, words = run.dirt()
    expect(acc == 0 and words == [0, 0, 0, 0], f"{tag}: {acc} non-zero accumulator bytes, status words 1/200/201/210 = {words} after the step")


def path(plan, name, c):
    # the path the configuration names, asserted: the solver mode, and the Jacobian kernel and its precision where the graph decides them
    jk, prec, mode = plan.jacobian_kernel, plan.edge_precision, plan.solver_mode
    kern = toks.get("kernel")
    want_mode = {"fused": 0, "lds": 0, "lds32": 1, "global": 2}.get(toks.get("solver"), 0)
    if name == "c3" and toks.get("order") == "natural":
        want_mode = 1                                          # (unpermuted, its factor fits LDS only as float: k_solve_lds<float>)
    if name in ("band300", "filled120"):
        want_mode = 3                                          # more than 255 free poses / filled in: dense
    if name == "band120":
        expect(mode in (1, 2), f"{name}: solver mode {mode}, not a refined float32 factor")
    elif name != "hubs3":                                      # (hubs3 is here for its loose tracks, ba_loose.hip)
        expect(mode == want_mode, f"{name}: solver mode {mode} != {want_mode}")
    if name == "g16":                                          # slot-uniform tiles: the forced kernel itself
        expect(jk == kern, f"{name}: {jk} != {kern}")
        if kern in ("k_stream", "k_edge2"):
            expect(prec == 6, f"{name}: edge precision {prec}")
    elif kern is None:                                         # (forced onto the fixtures a kernel may not fit their layout: reported)
        want = "k_etile" if name == "window_small" else "k_tile"
        expect(jk == want, f"{name}: {jk} != {want}")
        want = 4 if toks.get("prec") == "f32" else 8
        expect(prec == want, f"{name}: edge precision {prec} != {want}")
    if name == "hubs3":
        loc, kx = plan.array("trk_loc"), plan.array("kx")
        expect(sorted(kx[loc < 0]) == sorted(c["hubs"]), f"{name}: loose tracks {sorted(kx[loc < 0])}")
    return dict(kernel=jk, prec=prec, mode=mode)


def poisoned(plan, hp, pattern, other):
    nbytes = max(plan.workspace_bytes, 256)
    if pattern == "ff":
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        ws.fill_(0xFF)
    elif pattern == "one":
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)             # (workspace sizes are multiples of 256 bytes)
        ws.view(torch.float32).fill_(1.0)
    else:                                                                    # another plan's leftovers
        oc, ohp = other
        op = Plan(ohp.ii, ohp.jj, ohp.kk, ohp.poses.shape[1], ohp.patches.shape[1], oc["fixedp"])
        ws = torch.zeros(max(nbytes, op.workspace_bytes, 256), dtype=torch.uint8, device=DEV)
        orun = Run(ohp, op, ws)
        orun.step(split=False)
        orun.st.step(*orun.args(ep=-1e9))                                    # the last one a failed factorisation: status 1 left
        torch.cuda.synchronize()
        del orun
        op.close()
    run = Run(hp, plan, ws)
    run.init()
    return run


def failure_semantics(run, c, tag):
    # ba.py:9-13 and :324-325 through this child's solver (its refinement passes included), as test_gpu_parity has them for the
    # default and the dense solver
    st, D = run.st, 6 * run.plan.n
    a = run.args()
    st.step(*a, phase="reduce")
    good = st.system.clone()
    st.system.copy_(good)
    st.system[0] = -1e9                                          # a negative pivot (beyond the damping): failed factorisation, dX = 0
    st.step(*a, phase="solve_update")
    torch.cuda.synchronize()
    s, dx0 = st.status(), bool((st.dx == 0).all())
    ep = rel(run.Pout.cpu().numpy().astype(np.float64), run.hp.poses[0].cpu().numpy().astype(np.float64))
    expect(s == 1 and dx0 and ep < 1e-6, f"{tag}: negative pivot -> status {s}, dX all zero {dx0}, poses {ep:.3g} from Exp(0) G")
    st.system.copy_(good)
    st.system[D * D + 3] = float("nan")                          # a NaN in y: the factorisation succeeds, dX is NaN, one retry
    st.step(*a, phase="solve_update")
    torch.cuda.synchronize()
    s, nan = st.status(), bool(torch.isnan(st.dx).any())
    expect(s == 2 and nan, f"{tag}: NaN in y -> status {s}, NaN in dX {nan}")
    st.system.copy_(good)
    st.step(*a, phase="solve_update")
    torch.cuda.synchronize()
    o = dict(poses=run.Pout.cpu().numpy().astype(np.float64), patches=run.pout.cpu().numpy().astype(np.float64),
             dX=st.dx.cpu().numpy().astype(np.float64), status=st.status())
    r = vs_ref(o, c, tag + " the clean solve after them")
    check_dirt(run, tag + " after the failures")
    return r


loaded = {}
for name in CASES:
    c = loaded[name] = load(name)
    hp = HipProblem(c["d"])
    plan = Plan(hp.ii, hp.jj, hp.kk, hp.poses.shape[1], hp.patches.shape[1], c["fixedp"])
    m = meas[name] = dict(path=path(plan, name, c))
    c["gates"] = gates(name, plan.solver_mode)
    clean = Run(hp, plan)                                        # the same plan from a torch.zeros workspace
    b = clean.step()
    m["zeros"] = vs_ref(b, c, f"{name} zeros")
    del clean
    oname = "window_small" if name == "c1" else "c1"
    other = (loaded.get(oname) or load(oname),)
    other = (other[0], HipProblem(other[0]["d"]))
    for pattern in ("ff", "one", "leftovers"):
        tag = f"{name} {pattern}"
        run = poisoned(plan, hp, pattern, other)
        s0, x0 = run.st.status(), run.xchg_status()
        expect(s0 == 0 and x0 == 0, f"{tag}: after init bt_ba_status {s0}, bt_ba_xchg_status {x0}")           # (a)
        mp = m[pattern] = dict(init_status=[s0, x0])
        o1 = run.step()
        mp["ref"] = vs_ref(o1, c, tag + " step 1")                                                            # (b)
        mp["vs_zeros"] = vs_run(o1, b, tag + " step 1 vs zeros")                                              # (c)
        check_dirt(run, tag + " step 1")                                                                      # (e)
        o2 = run.step()
        mp["step2"] = vs_run(o2, o1, tag + " step 2 vs step 1")                                               # (d)
        check_dirt(run, tag + " step 2")
        o3 = run.step(split=False)
        mp["step3"] = vs_run(o3, o1, tag + " step 3 (bt_ba_step) vs step 1")
        check_dirt(run, tag + " step 3")
        run.st.step(*run.args(), phase="reduce")                                                              # (f)
        run.init()
        o4 = run.step(split=False)
        mp["split"] = vs_ref(o4, c, tag + " reduce, init, step")
        check_dirt(run, tag + " reduce, init, step")
        if "so_disp" in c and pattern == "ff":                   # structure-only through the same kernels, from a poisoned workspace
            sr = poisoned(plan, hp, pattern, other)
            mp["so"] = vs_ref(sr.step(split=False, so=True), c, tag + " structure-only", so=True)
            del sr
        if FAILURE and name == "c1" and pattern == "ff":
            mp["failures"] = failure_semantics(run, c, tag)
        del run
        torch.cuda.synchronize()
    plan.close()
print("RESULT " + json.dumps(dict(fails=fails, meas=meas)))
"""

FIXTURES = ["c1", "window_small", "c3"]
# (BT_FORCE tokens, cases, failure semantics) per child: every Jacobian-kernel and solver path.  g16 is a slot-uniform graph the forced
# wave-per-tile kernels take themselves; band120 a long thin band (refined float32 factor, unforced), filled120 / band300 dense
CONFIGS = {
    "default": ((), FIXTURES, False),                                  # k_tile / k_etile float64 + the barrier-free solver: the control
    "unforced-large": ((), ["band120", "filled120", "band300", "hubs3"], False),
    "fused": (("solver=fused",), FIXTURES, True),
    "lds": (("solver=lds",), FIXTURES, True),
    "lds-natural": (("solver=lds", "order=natural"), FIXTURES, False),
    "lds32": (("solver=lds32",), FIXTURES, True),
    "global": (("solver=global",), FIXTURES, True),
    "k_etile": (("kernel=k_etile",), FIXTURES + ["g16"], False),
    "k_stream": (("kernel=k_stream",), FIXTURES + ["g16"], False),
    "k_edge2": (("kernel=k_edge2",), FIXTURES + ["g16"], False),
    "f32-wide0": (("prec=f32", "wide=0"), FIXTURES, False),
    "f32-wide1": (("prec=f32", "wide=1"), FIXTURES, False),
}
# (c) / (d): two steps of the same inputs in different workspaces differ only by the order of the fp64 atomics: dX within DX_SAME, the
# new poses and patches within STATE_SAME, relative.  Measured on an MI355X: [S | y] <= 3.5e-16 apart; dX and state bit for bit the same
# through the float64 factors, dX 1.3e-8 / state 3.1e-9 through the refined float32 ones (the atomics' last bit flips a float32 rounding)
DX_SAME, STATE_SAME = 1e-7, 3e-8


@pytest.mark.parametrize("config", list(CONFIGS))
def test_steps_from_a_poisoned_workspace(config):
    import force
    toks, cases, failure = CONFIGS[config]
    e = force.env_with(*toks)
    arg = json.dumps([cases, failure, DX_SAME, STATE_SAME])
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + SCRIPT, arg], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(json.dumps(res["meas"]))
    assert not res["fails"], "\n".join(res["fails"][:40])
