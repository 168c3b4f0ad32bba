"""tests/solver_faults.py without a GPU: the restated solve against the oracle's, its two failure exits, the problems with one
failing pivot against the oracle, and the fault catalogue against the plan's own pattern."""
import os

import numpy as np
import pytest
import torch

from batrack_amd import graphgen
from batrack_amd.plan import Plan
from edge_problems import band_120
from solver_faults import (NEG, backward_error, damped, faults, is_wide, localised_failure, oracle_step, pattern,
                           solve_reference)

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def load(name):
    d = dict(np.load(os.path.join(GOLD, name + ".npz")))
    return d, (int(d["fixedp"]) if "fixedp" in d else 1)


def flat(S, y):
    return np.concatenate([np.tril(S).reshape(-1), y])          # as Stepper.system holds it: the lower triangle, then y


_REF = {}


def reference(name):
    """The oracle's step on a fixture, computed once and left unchanged."""
    if name not in _REF:
        d, fp = load(name)
        _REF[name] = (d, fp, oracle_step(d, fp))
    return _REF[name]


@pytest.mark.parametrize("name", ["c1", "c1_rough", "window_small"])
def test_solve_reference_matches_the_oracle(name):
    d, fp, r = reference(name)
    D = r["y"].size
    status, dX = solve_reference(flat(r["S"], r["y"]), D, 10.0)
    assert status == 0 and not r["failed"]
    assert rel(dX, r["dX"].reshape(-1)) < 1e-10


def test_backward_error_and_damping_by_hand():
    A = np.array([[2.0, 0.0], [0.0, 2.0]])
    assert backward_error(A, [1.0, 2.0], [2.0, 4.0]) == 0.0
    assert backward_error(A, [1.0, 2.0], [2.0, 5.0]) == 1.0 / (2.0 * 2.0 + 5.0)
    # [S | y] with the lower triangle stored (the 7 above the diagonal is not part of S): A = sym + diag(ep + lm diag S)
    A, y = damped(np.array([4.0, 7.0, 1.0, 3.0, 5.0, 6.0]), 2, 10.0, lm=0.5)
    assert A.tolist() == [[16.0, 1.0], [1.0, 14.5]] and y.tolist() == [5.0, 6.0]


def test_solve_reference_failed_factorisation_gives_zeros():
    d, fp, r = reference("c1")
    D = r["y"].size
    status, dX = solve_reference(flat(r["S"], r["y"]), D, NEG)
    assert status == 1 and dX.shape == (D,) and np.all(dX == 0)
    bad = oracle_step(d, fp, ep=NEG)
    assert bad["failed"] and np.all(bad["dX"] == 0)


@pytest.mark.parametrize("k", [0, 3, 41])
def test_solve_reference_nan_in_y_is_retried(k):
    d, fp, r = reference("c1")
    D = r["y"].size
    y = r["y"].copy()
    y[k] = np.nan
    status, dX = solve_reference(flat(r["S"], y), D, 10.0)
    assert status == 2 and np.isnan(dX[k])


@pytest.mark.parametrize("where", ["diag", "off"])
def test_solve_reference_reports_a_nan_pivot(where):
    d, fp, r = reference("c1")
    D = r["y"].size
    S = r["S"].copy()
    if where == "diag":
        S[D - 1, D - 1] = np.nan
    else:
        S[D - 1, 2] = np.nan                                     # (stored triangle: reaches the pivot of its row)
    status, dX = solve_reference(flat(S, r["y"]), D, 10.0)
    assert status == 1 and np.all(dX == 0)


@pytest.mark.parametrize("name", ["c1", "window_small"])
def test_localised_failure_fails_at_one_pose_only(name):
    d, fp, r = reference(name)
    n = r["y"].size // 6
    for p in range(n):
        w, ep = localised_failure(d, p, fp)
        assert ep < 0 and np.float32(ep) == ep
        bad = oracle_step(d, fp, weights=w, ep=ep)
        S = bad["S"]
        assert np.all(S[6 * p:6 * p + 6] == 0) and np.all(S[:, 6 * p:6 * p + 6] == 0)      # block row and column p exactly 0
        assert bad["failed"] and np.all(bad["dX"] == 0)
        ok = oracle_step(d, fp, weights=w, ep=abs(ep))
        assert not ok["failed"] and np.all(ok["dX"][p] == 0) and np.isfinite(ok["dX"]).all()
        # the only failing pivot: without pose p's rows and columns the system factors with that negative ep
        keep = np.delete(np.arange(6 * n), np.arange(6 * p, 6 * p + 6))
        A, _ = damped(flat(S, bad["y"]), 6 * n, ep)
        assert int(torch.linalg.cholesky_ex(A[keep][:, keep])[1]) == 0, p


def _host_plans():
    d, fp = load("c1")
    yield "c1", Plan(d["ii"], d["jj"], d["kk"], d["poses"].shape[0], d["patches"].shape[0], fp, upload=False), None
    d, fp = load("window_small")
    yield "window_small", Plan(d["ii"], d["jj"], d["kk"], d["poses"].shape[0], d["patches"].shape[0], fp, upload=False), None
    g = graphgen.make_config("C3", seed=0)
    yield "c3", Plan(g.ii, g.jj, g.kk, g.poses.shape[0], g.patches.shape[0], 1, upload=False), None
    ii, jj, kk, N, P = band_120(filled=True)
    yield "filled120", Plan(ii, jj, kk, N, P, 1, upload=False), True
    g = graphgen.make_graph(258, 16, 6, seed=21)
    yield "band258", Plan(g.ii, g.jj, g.kk, 258, g.patches.shape[0], 1, upload=False), None


@pytest.mark.parametrize("case", ["c1", "window_small", "c3", "filled120", "band258"])
def test_fault_catalogue_lies_in_the_plans_pattern(case):
    name, pl, wide = next(c for c in _host_plans() if c[0] == case)
    A = {k: pl.array(k) for k in ("perm", "col_ptr", "row_idx", "blk_src")}
    n, D = pl.n, 6 * pl.n
    wide = is_wide(A, D) if wide is None else wide
    assert wide == (case in ("filled120", "band258"))
    cat = faults(A, D, wide=wide)
    pat = pattern(A, D, wide)
    if not wide:
        assert len(pat) == pl.nnz_blocks
    by = {}
    for f in cat:
        by.setdefault(f.kind, []).append(f)
    assert sorted(by) == ["nan_diag", "nan_off", "nan_y", "neg"]
    for kind in ("neg", "nan_diag", "nan_y"):                    # every (pose, scalar) once per kind
        assert sorted(f.k for f in by[kind]) == list(range(D)), kind
    for f in by["neg"] + by["nan_diag"]:
        assert f.index == f.k * D + f.k and f.status == 1
    assert all(f.value == NEG for f in by["neg"]) and all(np.isnan(f.value) for f in by["nan_diag"] + by["nan_off"] + by["nan_y"])
    for f in by["nan_y"]:
        assert f.index == D * D + f.k < D * D + D and f.status == 2
    seen = set()
    for f in by["nan_off"]:
        r, c = divmod(f.index, D)
        assert 0 <= f.index < D * D and r > c and r // 6 > c // 6          # strictly below the diagonal block: a stored element
        assert (r // 6, c // 6) in pat and f.k == r and f.status == 1
        seen.add((r // 6, c // 6))
    assert len(seen) == len(by["nan_off"])                        # one element a block
    if wide:
        rows = {b[0] for b in seen}
        assert {1, n // 2, n - 1} <= rows
    else:
        assert seen == {b for b in pat if b[0] != b[1]}           # every structurally non-zero off-diagonal block
        # (the elements vary: every scalar of a block row and column is hit somewhere in a plan of more than a few blocks)
        if len(seen) >= 36:
            assert {divmod(f.index, D)[0] % 6 for f in by["nan_off"]} == set(range(6))
    pl.close()
