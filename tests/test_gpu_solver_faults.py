"""-m gpu: the reduced solvers' failure paths at every pivot, on every route (tests/solver_faults.py has the contract and the catalogue).

ba.py:9-13, :60-70, :323-325: a non-positive or NaN pivot gives dX = 0 and status 1, a NaN in dX one retry at lm = 1e-3 and status 2.
The other tests fail the FIRST pivot (ep = -1e9, system[0]) or poison y[3]; where a failure is noticed differs from solver to solver
(thread 0, lane 0 of the diagonal wave, row wave 0 of a column after it has factored the published block itself, a flag carried
through global memory across the dense solver's launches), so here
  (a) every scalar's pivot, one element of every structurally non-zero off-diagonal block and every entry of y is broken in turn, in
      the [S | y] the plan's own reduce phase produced, through the split phases of the barrier-free, fused, two-phase, float LDS
      and global solvers; clean solves in between must give the first clean dX again and leave the workspace clear
  (b) the dense solver at D % 48 = 0, 6 and 42 (backward error), its faults in the first two panels, the last full one and the ragged
      one, on a band and on a filled-in graph, and one whole step at the ABI's limit of 2048 free poses
  (c) a real problem whose only failing pivot is one chosen pose, through whole steps: the fused solve + update launch
      (k_solve_update, reached by bt_ba_step alone) against the two launches, bit for bit, and against the oracle
  (d) the float64 solvers on badly scaled systems S' = diag(s) S diag(s), s = 10^U[-2, 2]: backward error
Only values of [S | y] inside the plan's pattern, weights and ep are written; no table, pattern or status word.  BT_FORCE is read once
per process: one child interpreter per configuration, one at a time; a child that did not end with exit status 0 is the last one
this module starts.

Backward-error gate of (b) and (d): 2^-23 = 1.19e-7, derived, not tuned — dX is stored as float32, |x^ - x| <= 2^-24 |x| componentwise,
so the residual is at most 2^-24 ||A|| ||x||; a float64 Cholesky adds O(D 2^-53); the gate is twice that bound.
Measured on an MI355X: see MEASURED below."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import torch
import oracle
import force
import solver_faults as sf
from gpu_util import DEV, HipProblem
from edge_problems import band_120_problem
from batrack_amd import graphgen
from batrack_amd.plan import Plan, Stepper

SPEC = json.loads(sys.argv[1])
OUT = sys.argv[2] if len(sys.argv) > 2 else None
DX_SAME = SPEC["dx_same"]
GATE_BE = 2.0 ** -23
toks = force.tokens()
fails, meas, saved = [], {}, {}
GOLD = os.path.join(ROOT, "tests", "golden")
f64 = lambda a: np.asarray(a, np.float32).astype(np.float64)


def expect(ok, what):
    if not ok:
        fails.append(what)


def from_graph(g):
    return dict(poses=f64(g.poses), patches=f64(g.patches), mono=f64(g.mono_disp), intrinsics=f64(g.intrinsics), targets3=f64(g.targets3),
                weights=f64(g.weights), weights_pose=f64(g.weights_pose), ii=g.ii, jj=g.jj, kk=g.kk, bounds=np.asarray(g.bounds, np.float64))


def load(name):
    # -> inputs, fixedp
    if name in ("c1", "window_small"):
        d = dict(np.load(os.path.join(GOLD, name + ".npz")))
        return d, (1 if name == "c1" else int(d["fixedp"]))
    if name == "c3":
        return from_graph(graphgen.make_config("C3", seed=0)), 1
    if name == "filled120":
        return band_120_problem(filled=True), 1
    if name == "eight_tiles":                                    # tests/test_gpu_solve_update_fused.py's: 8 tiles of 64 tracks
        return from_graph(graphgen.make_graph(8, 64, 5, seed=4)), 1
    if name.startswith("band"):                                  # tests/test_gpu_parity.py's wide bands, other lengths
        return from_graph(graphgen.make_graph(int(name[4:]), 16, 6, seed=21)), 1
    if name.startswith("thin"):                                  # 4 tracks a frame, seen from 3 frames
        return from_graph(graphgen.make_graph(int(name[4:]), 4, 3, seed=21)), 1
    raise KeyError(name)


class Run:
    # one plan, one workspace, the caller's buffers
    def __init__(self, d, fixedp):
        self.d, self.fixedp = d, fixedp
        self.hp = hp = HipProblem(d)
        self.plan = Plan(hp.ii, hp.jj, hp.kk, hp.poses.shape[1], hp.patches.shape[1], fixedp)
        self.st = Stepper(self.plan, DEV)
        self.P = hp.poses[0].contiguous()
        self.pat = hp.patches.reshape(-1, 3).contiguous()
        self.Pout, self.pout = torch.empty_like(self.P), torch.empty_like(self.pat)
        self.lay = self.plan.ws_layout
        self.n, self.D = self.plan.n, 6 * self.plan.n
        self.w = hp.w["weights_pose"][0].contiguous()

    def args(self, ep=10.0, w=None):
        hp, tg = self.hp, self.hp.t3[0]
        return (self.P, self.pat, hp.mono.reshape(-1), hp.intr[0], tg, tg.stride(0), self.w if w is None else w,
                self.Pout, self.pout, hp.bounds, 1e-4, ep, 0.05, "huber", False)

    def arrays(self):
        return {k: self.plan.array(k) for k in ("perm", "col_ptr", "row_idx", "blk_src")}

    def dirt(self):
        # what a completed step must leave behind (tests/test_gpu_workspace.py): the accumulators zero, the solvers' flags 0
        lay, ws = self.lay, self.st.ws
        acc = int(torch.count_nonzero(ws[lay["sys"]:lay["sys"] + lay["zero_bytes"]]))
        words = ws[lay["status"]:lay["status"] + 1024].view(torch.int32)[[1, 200, 201, 210]].cpu().tolist()
        return acc, words

    def close(self):
        del self.st
        self.plan.close()


def check_dirt(run, tag):
    acc, words = run.dirt()
    expect(acc == 0 and words == [0, 0, 0, 0], f"{tag}: {acc} non-zero accumulator bytes, status words 1/200/201/210 = {words} after the step")


def drel(a, b):
    return (a - b).norm() / b.norm().clamp_min(1e-300)


def route(run, name, want_mode):
    # the route the configuration names, asserted as tests/test_gpu_workspace.py does: the forced token and the plan's solver mode
    expect(toks.get("solver") == SPEC.get("solver"), f"{name}: BT_FORCE solver token {toks.get('solver')} != {SPEC.get('solver')}")
    expect(run.plan.solver_mode == want_mode, f"{name}: solver mode {run.plan.solver_mode} != {want_mode}")


def failed_step(d, fixedp):
    # a failed solve moves the depths by Q w' alone (test_cholesky_failure_gives_zero_pose_update's reference)
    r = oracle.ba_step(d["poses"], d["patches"], d["mono"], d["intrinsics"], d["targets3"], d["weights_pose"], d["ii"], d["jj"], d["kk"],
                       d["bounds"], fixedp=fixedp, ep=-1e9)
    expect(r["failed"], "the oracle does not fail with ep = -1e9")
    return torch.as_tensor(r["patches_out"], dtype=torch.float64, device=DEV)


def sweep(run, name, cat, bitwise):
    # every fault of `cat` in turn in the [S | y] of one reduce; a clean solve after every 16th and after the last
    st, D = run.st, run.D
    a = run.args()
    st.step(*a, phase="reduce")
    torch.cuda.synchronize()
    good = st.system.clone()
    m = meas[name] = dict(D=D, faults={}, clean_solves=0, clean_dx=0.0, clean_bitwise=True)
    first = [None]

    def clean(tag):
        st.system.copy_(good)
        st.step(*a, phase="solve_update")
        torch.cuda.synchronize()
        s = st.status()
        expect(s == 0, f"{tag}: status {s}")
        if first[0] is None:
            first[0] = st.dx.clone()
            expect(bool(torch.isfinite(first[0]).all()), f"{tag}: dX not finite")
        else:
            e, same = float(drel(st.dx.double(), first[0].double())), bool(torch.equal(st.dx, first[0]))
            m["clean_dx"], m["clean_bitwise"] = max(m["clean_dx"], e), m["clean_bitwise"] and same
            expect(e <= DX_SAME and (same or not bitwise), f"{tag}: dX {e:.3g} from the first clean solve's, bit for bit {same}")
        m["clean_solves"] += 1
        check_dirt(run, tag)

    clean(f"{name} first clean solve")
    P_in, ref_pat = run.P.double(), failed_step(run.d, run.fixedp)
    t0 = time.perf_counter()
    for i, f in enumerate(cat):
        st.system.copy_(good)
        st.system[f.index] = f.value
        st.step(*a, phase="solve_update")
        s = st.status()
        tag = f"{name} {f.kind} at pose {f.k // 6} scalar {f.k % 6} (system[{f.index}])"
        if f.status == 1:
            nz, ep, epat = torch.stack([(st.dx != 0).sum().double(), drel(run.Pout.double(), P_in), drel(run.pout.double(), ref_pat)]).tolist()
            expect(s == 1 and nz == 0 and ep < 1e-6 and epat < 1e-5,
                   f"{tag}: status {s}, {int(nz)} entries of dX not zero, poses {ep:.3g} from the inputs, patches {epat:.3g} from Q w'")
        else:
            nan_k = bool(torch.isnan(st.dx.reshape(-1)[f.k]))
            expect(s == 2 and nan_k, f"{tag}: status {s}, isnan(dX[{f.k}]) {nan_k}")
        m["faults"][f.kind] = m["faults"].get(f.kind, 0) + 1
        if (i + 1) % 16 == 0 or i == len(cat) - 1:
            clean(f"{name} clean solve after fault {i + 1} ({f.kind} at {f.k})")
    m["sweep_seconds"] = round(time.perf_counter() - t0, 3)


def part_a():
    want_mode = {"fused": 0, "lds": 0, "lds32": 1, "global": 2}.get(toks.get("solver"), 0)
    for name in SPEC["cases"]:
        run = Run(*load(name))
        route(run, name, want_mode)
        # bit for bit where test_solver_gives_the_same_answer_every_time asserts it: the unforced solver on C1 and C3
        sweep(run, name, sf.faults(run.arrays(), run.D, wide=False), bitwise="solver" not in toks and name in ("c1", "c3"))
        run.close()


def dense_run(name):
    run = Run(*load(name))
    route(run, name, 3)
    n = run.n
    expect(run.plan.nnz_blocks == n * (n + 1) // 2 and np.array_equal(run.plan.array("perm"), np.arange(n)), f"{name}: the plan is not wide")
    return run


def solve_from(run, system, tag, ep=10.0):
    # [S | y] := system, one solve -> status, backward error of dX against the damped system built on the CPU
    st = run.st
    st.system.copy_(system)
    st.step(*run.args(ep=ep), phase="solve_update")
    torch.cuda.synchronize()
    s = st.status()
    A, y = sf.damped(system.cpu(), run.D, ep)
    be = sf.backward_error(A, st.dx.cpu().double(), y)
    expect(s == 0 and be < GATE_BE, f"{tag}: status {s}, backward error {be:.3g} (gate {GATE_BE:.3g})")
    check_dirt(run, tag)
    return be


def part_b_accuracy():
    for frames in SPEC["frames"]:
        name = f"band{frames}"
        run = dense_run(name)
        expect(run.n == frames - 1, f"{name}: {run.n} free poses")
        run.st.step(*run.args(), phase="reduce")
        torch.cuda.synchronize()
        good = run.st.system.clone()
        meas[name] = dict(D=run.D, D_mod_48=run.D % 48, backward_error=solve_from(run, good, name))
        run.close()


def part_b_faults():
    name = SPEC["case"]
    run = dense_run(name)
    D = run.D
    full = (D // 48) * 48
    # first and last row of the first two panels, the last full panel's last row, the ragged panel's first and last row
    rows = {0, 47, 48, 95, full - 1, full, D - 1}
    expect(D % 48 != 0 and (name != "band258" or sorted(rows) == [0, 47, 48, 95, 1535, 1536, 1541]), f"{name}: D = {D}, rows {sorted(rows)}")
    cat = [f for f in sf.faults(run.arrays(), D, wide=True) if f.kind == "nan_off" or f.k in rows]
    sweep(run, name, cat, bitwise=False)
    run.close()


def part_b_limit():
    name = "thin2049"
    run = dense_run(name)
    st, D = run.st, run.D
    expect(run.n == 2048 and D == 12288, f"{name}: {run.n} free poses")
    a = run.args()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    st.step(*a)                                                  # one whole step
    ev1.record()
    torch.cuda.synchronize()
    s, dx = st.status(), st.dx.double().reshape(-1).clone()
    finite = bool(torch.isfinite(dx).all())
    check_dirt(run, name)
    # the residual in float64 on the device ([S | y] is 1.2 GB) against the system of a second reduce of the same inputs (the
    # same [S | y] up to the order of the fp64 atomics, 1e-15)
    st.step(*a, phase="reduce")
    torch.cuda.synchronize()
    S = st.system[:D * D].view(D, D)
    y = st.system[D * D:D * D + D].clone()
    A = torch.tril(S)
    A += torch.tril(S, -1).T
    A.diagonal().add_(10.0 + 1e-4 * S.diagonal())
    be = sf.backward_error(A, dx, y)
    meas[name] = dict(D=D, status=s, step_ms=round(ev0.elapsed_time(ev1), 1), backward_error=be)
    expect(s == 0 and finite and be < GATE_BE, f"{name}: status {s}, dX finite {finite}, backward error {be:.3g} (gate {GATE_BE:.3g})")
    del A, S
    run.close()


def part_c():
    # whole steps (bt_ba_step) of a problem whose only failing pivot is free pose p
    for name in SPEC["cases"]:
        d, fp = load(name)
        run = Run(d, fp)
        st, n = run.st, run.n
        perm = run.plan.array("perm")
        ps = list(range(n)) if name != "eight_tiles" else [int(perm[0]), int(perm[n // 2]), int(perm[n - 1])]     # first, middle, last in factor order
        saved[name + ".kernel"] = np.asarray(run.plan.jacobian_kernel)
        m = meas[name] = dict(poses=ps, ep=[], err_poses=0.0, err_patches=0.0)
        for p in ps:
            w, ep = sf.localised_failure(d, p, fp)
            ref = sf.oracle_step(d, fp, weights=w, ep=ep)
            expect(ref["failed"] and not sf.oracle_step(d, fp, weights=w, ep=abs(ep))["failed"], f"{name} pose {p}: the oracle's verdicts")
            wd = torch.as_tensor(np.asarray(w, np.float32), device=DEV).contiguous()
            a = run.args(ep=ep, w=wd)
            st.step(*a)
            torch.cuda.synchronize()
            s, dx = st.status(), st.dx.cpu().numpy()
            P, X = run.Pout.cpu().numpy(), run.pout.cpu().numpy()
            e1 = float(np.linalg.norm(P - ref["poses_out"]) / np.linalg.norm(ref["poses_out"]))
            e2 = float(np.linalg.norm(X - ref["patches_out"]) / np.linalg.norm(ref["patches_out"]))
            m["ep"].append(ep); m["err_poses"] = max(m["err_poses"], e1); m["err_patches"] = max(m["err_patches"], e2)
            expect(s == 1 and bool(np.all(dx == 0)) and e1 < 1e-6 and e2 < 1e-5,
                   f"{name} pose {p} (ep {ep:.4g}): status {s}, {int(np.count_nonzero(dx != 0))} entries of dX not zero, poses {e1:.3g}, patches {e2:.3g} from the oracle")
            check_dirt(run, f"{name} pose {p}")
            for k, v in (("status", np.asarray(s)), ("dx", dx), ("poses", P), ("patches", X)):
                saved[f"{name}.{p}.{k}"] = v
            if p == ps[0]:                                       # which kernels a timed step of these arguments launches
                ms = st.step_timed(*a)
                torch.cuda.synchronize()
                saved[name + ".ran"] = np.asarray([ms[k] > 0 for k in ("tile", "pair_finalize", "solve", "update")])
        saved[name + ".poses_list"] = np.asarray(ps)
        run.close()


def part_d():
    for name in SPEC["cases"]:
        run = Run(*load(name))
        route(run, name, 3 if name == "filled120" else 0)
        st, D = run.st, run.D
        st.step(*run.args(), phase="reduce")
        torch.cuda.synchronize()
        good = st.system.clone()
        m = meas[name] = dict(D=D, backward_error=[])
        for seed in (0, 1):
            s = torch.as_tensor(10.0 ** np.random.default_rng(seed).uniform(-2.0, 2.0, D), device=DEV)
            scaled = good.clone()
            scaled[:D * D].view(D, D).mul_(s[:, None] * s[None, :])
            scaled[D * D:D * D + D].mul_(s)
            m["backward_error"].append(solve_from(run, scaled, f"{name} scaled, draw {seed}"))
        m["unscaled"] = solve_from(run, good, f"{name} unscaled")
        run.close()


{"a": part_a, "b_accuracy": part_b_accuracy, "b_faults": part_b_faults, "b_limit": part_b_limit, "c": part_c, "d": part_d}[SPEC["part"]]()
if OUT:
    np.savez(OUT, **saved)
print("RESULT " + json.dumps(dict(fails=fails[:200], nfails=len(fails), meas=meas)))
"""

# test_gpu_workspace.py's: two solves of the same [S | y] — bit for bit through the float64 factors, 1.3e-8 through the refined float32 ones
DX_SAME = 1e-7

# MEASURED (MI355X), next to their gates:
#   backward error, gate 2^-23 = 1.19e-7
#     (b) dense, clean: band257 (D % 48 = 0) 2.6e-9, band258 (6) 2.3e-9, band264 (42) 2.9e-9; thin2049 (D = 12288) 2.5e-9, its
#         whole step 128 ms
#     (d) scaled, two draws: c3 barrier-free 2.9e-12 / 1.3e-12, filled120 dense 1.8e-12 / 1.1e-12, c1 fused and c1 two-phase
#         1.7e-12 / 8.3e-12 (the large scales dominate ||A|| ||x||); the same systems unscaled 2.6e-9 .. 3.8e-9
#   (a) clean solves between the faults: dX bit for bit the first clean solve's on every route, the refined float32 ones included
#       (gate DX_SAME); faults per route: c1 147, window_small 375, c3 1547 (3 D + one per off-diagonal block of the factor);
#       the c3 sweep takes 0.33 .. 0.38 s a child, unthinned
#   (c) poses <= 1.7e-8 (gate 1e-6) and patches <= 2.6e-11 (gate 1e-5) from the oracle's failed step
_STOPPED = []


def child(spec, toks=(), out=None, timeout=300):
    """One child interpreter under these BT_FORCE tokens -> its RESULT.  After a child that did not exit with status 0 no other starts."""
    import force
    if _STOPPED:
        pytest.fail(f"not started: an earlier child of this module ended with {_STOPPED[0]}")
    solver = dict(t.split("=") for t in toks).get("solver")
    arg = json.dumps(dict(spec, solver=solver, dx_same=DX_SAME))
    cmd = [sys.executable, "-c", f"ROOT = {ROOT!r}\n" + SCRIPT, arg] + ([out] if out else [])
    try:
        r = subprocess.run(cmd, env=force.env_with(*toks), capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _STOPPED.append(f"a time-out after {timeout} s ({spec})")
        raise
    if r.returncode != 0:
        _STOPPED.append(f"exit status {r.returncode} ({spec})")
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(json.dumps(res["meas"]))
    assert not res["fails"], f"{res['nfails']} failures:\n" + "\n".join(res["fails"][:40])
    return res["meas"]


FIXTURES = ["c1", "window_small", "c3"]
INJECTED = {
    "default": ((), FIXTURES),                                   # the barrier-free solver (k_solve_pipe)
    "fused": (("solver=fused",), FIXTURES),
    "lds": (("solver=lds",), FIXTURES),
    "lds32": (("solver=lds32",), FIXTURES[:2]),
    "global": (("solver=global",), FIXTURES[:2]),
}


@pytest.mark.parametrize("config", list(INJECTED))
def test_injected_faults_through_the_split_phases(config):
    """(a).  c1: 7 free poses; window_small: the real window; c3: 63 free poses, two columns a level.  Per fixture 3 D faults on the
    diagonal and in y and one per off-diagonal block of the factor."""
    toks, cases = INJECTED[config]
    m = child(dict(part="a", cases=cases), toks)
    for name in cases:
        f = m[name]["faults"]
        assert f["neg"] == f["nan_diag"] == f["nan_y"] == m[name]["D"] and f["nan_off"] > 0
        assert m[name]["clean_solves"] == 1 + -(-sum(f.values()) // 16)          # the first, one after every 16th fault and after the last


def test_dense_solver_backward_error_at_full_and_ragged_last_panels():
    """(b) accuracy: bands of 257, 258 and 264 frames, D % 48 = 0, 6 and 42."""
    m = child(dict(part="b_accuracy", frames=[257, 258, 264]))
    assert [m[f"band{f}"]["D_mod_48"] for f in (257, 258, 264)] == [0, 6, 42]


@pytest.mark.parametrize("case", ["band258", "filled120"])
def test_dense_solver_faults_in_every_kind_of_panel(case):
    """(b) faults: rows 0, 47, 48, 95, the last full panel's last row and the ragged panel's first and last row."""
    m = child(dict(part="b_faults", case=case))
    f = m[case]["faults"]
    assert f["neg"] == f["nan_diag"] == f["nan_y"] == 7 and f["nan_off"] >= 3


def test_dense_solver_at_the_limit_of_2048_free_poses():
    """(b) the limit: one whole step of a thin band of 2049 frames, D = 12288 ([S | y] and the factor 1.2 GB each)."""
    child(dict(part="b_limit"), timeout=180)


def same_bits(a, b):
    """tests/test_gpu_solve_update_fused.py's: equal bit for bit, NaN exactly where the other has NaN."""
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and a[~na].tobytes() == b[~nb].tobytes()


def test_single_failing_pivot_through_whole_steps(tmp_path):
    """(c).  The fused solve + update launch (unforced, on the k_tile fixtures) against upd=split and against the oracle."""
    cases = ["c1", "window_small", "eight_tiles"]
    out = {}
    for tag, toks in (("fused", ()), ("split", ("upd=split",))):
        path = str(tmp_path / (tag + ".npz"))
        child(dict(part="c", cases=cases), toks, out=path)
        out[tag] = dict(np.load(path))
    fused, split = out["fused"], out["split"]
    for name in cases:
        # the timed step: the fused launch is recorded under the solver's event pair, the update's entry stays 0.  (window_small
        # takes k_etile, whose update is a launch of its own on every route.)
        tile = str(fused[name + ".kernel"]) == "k_tile"
        assert tile == (name != "window_small")
        assert fused[name + ".ran"].tolist() == [True, True, True, not tile], (name, fused[name + ".ran"])
        assert split[name + ".ran"].tolist() == [True, True, True, True], (name, split[name + ".ran"])
        ps = fused[name + ".poses_list"].tolist()
        assert ps == split[name + ".poses_list"].tolist() and len(ps) >= 3
        for p in ps:
            assert int(fused[f"{name}.{p}.status"]) == int(split[f"{name}.{p}.status"]) == 1
            for what in ("dx", "poses", "patches"):
                assert same_bits(fused[f"{name}.{p}.{what}"], split[f"{name}.{p}.{what}"]), (name, p, what)


SCALED = {
    "default": ((), ["c3", "filled120"]),                        # the barrier-free solver; the dense one
    "fused": (("solver=fused",), ["c1"]),
    "lds": (("solver=lds",), ["c1"]),
}


@pytest.mark.parametrize("config", list(SCALED))
def test_float64_solvers_on_badly_scaled_systems(config):
    """(d).  S' = diag(s) S diag(s), y' = s y, s = 10^u, u ~ U[-2, 2] per scalar, two draws."""
    toks, cases = SCALED[config]
    child(dict(part="d", cases=cases), toks)
