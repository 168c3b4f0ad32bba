"""What a reduced-system solver owes its caller, and where to break a system to find out (no GPU here).

Every solver of ba_solve.hip and ba_dense.hip implements ba.py:9-13, :60-70 and :323-325: a non-positive or NaN pivot gives
dX = 0 and status 1; a NaN in dX one retry at lm = 1e-3 and status 2.  `solve_reference` restates that for a dense [S | y] as
Stepper.system holds it, `faults` lists one-value changes of such a system that must take each of those exits — at every pivot,
inside every structurally non-zero block, in every entry of y —, `localised_failure` builds a real problem whose only failing
pivot is one chosen pose.  tests/test_solver_faults_cpu.py checks these helpers, tests/test_gpu_solver_faults.py uses them."""
from collections import namedtuple

import numpy as np
import torch

import oracle

NEG = -1e9                                     # a pivot beyond any damping of the fixtures (diag S <= 1e7, ep = 10)


def _parts(system, D):
    v = torch.as_tensor(np.asarray(system) if not isinstance(system, torch.Tensor) else system).detach().to("cpu", torch.float64).reshape(-1)
    return v[:D * D].reshape(D, D), v[D * D:D * D + D]


def damped(system, D, ep, lm=1e-4):
    """A = sym(tril S) + diag(ep + lm diag S) and y of a flat [S | y] (lower triangle of S stored), float64 on the CPU."""
    S, y = _parts(system, D)
    low = torch.tril(S)
    A = low + torch.tril(S, -1).T
    dg = torch.diagonal(S)
    A = A + torch.diag(ep + lm * dg)
    return A, y.clone()


def solve_reference(system, D, ep):
    """-> (status, dX [D] float64): ba.py:60-70 with ba.py:9-13 and :323-325 around it, by the reference's own routine."""
    ep = float(ep)
    for attempt, lm in enumerate((1e-4, 1e-3)):
        A, y = damped(system, D, ep, lm)
        L, info = torch.linalg.cholesky_ex(A)
        if int(info) != 0:
            return 1, np.zeros(D)
        dX = torch.cholesky_solve(y[:, None], L)[:, 0]
        if not bool(torch.isnan(dX).any()):
            return (0 if attempt == 0 else 2), dX.numpy()
    return 2, dX.numpy()


def backward_error(A, x, y):
    """||y - A x||_inf / (||A||_inf ||x||_inf + ||y||_inf), float64 (A, x, y: numpy arrays or torch tensors on any device)."""
    A, x, y = (torch.as_tensor(t).to(torch.float64) for t in (A, x, y))
    x, y = x.reshape(-1).to(A.device), y.reshape(-1).to(A.device)
    r = (y - A @ x).abs().max()
    return float(r / (A.abs().sum(1).max() * x.abs().max() + y.abs().max()))


# index: into the flat system; k: the caller-order scalar the fault belongs to (its pivot, its entry of y; the row of a block's
# element); status: what the solve must report — 1 with dX == 0, or 2 with isnan(dX[k])
Fault = namedtuple("Fault", "kind index value status k")


def pattern(plan_arrays, D, wide):
    """{(block row, block column)} of the caller-order lower triangle that the plan's solver reads, from perm / col_ptr / row_idx."""
    n = D // 6
    if wide:
        return {(r, c) for r in range(n) for c in range(r + 1)}
    perm, col_ptr, row_idx = (np.asarray(plan_arrays[k]) for k in ("perm", "col_ptr", "row_idx"))
    out = set()
    for j in range(n):
        for b in range(int(col_ptr[j]), int(col_ptr[j + 1])):
            x, y = int(perm[row_idx[b]]), int(perm[j])
            out.add((max(x, y), min(x, y)))
    return out


def is_wide(plan_arrays, D):
    """A plan of more than 255 free poses carries no block tables: identity order, every lower block (ba_dense.hip)."""
    return D // 6 > 255 or np.asarray(plan_arrays["row_idx"]).size == 0


def faults(plan_arrays, D, wide=None):
    """The catalogue for a plan of D = 6 n scalars (plan_arrays: perm, col_ptr, row_idx, blk_src as Plan.array gives them).
    wide: the plan's solver is the dense one (solver mode 3) — by default, what `is_wide` says."""
    n = D // 6
    wide = is_wide(plan_arrays, D) if wide is None else bool(wide)
    out = []
    for k in range(D):
        out.append(Fault("neg", k * D + k, NEG, 1, k))
    for k in range(D):
        out.append(Fault("nan_diag", k * D + k, float("nan"), 1, k))
    if wide:
        # one element in the first, a middle and the last block row that has blocks below the diagonal
        blocks = sorted({(1, 0), (n // 2, n // 4), (n - 1, 0), (n - 1, n - 2)} if n > 1 else set())
        for i, (rn, cn) in enumerate(b for b in blocks if b[0] > b[1]):
            r, c = (5, 0, 2, 3)[i % 4], (0, 5, 3, 1)[i % 4]
            out.append(Fault("nan_off", (6 * rn + r) * D + 6 * cn + c, float("nan"), 1, 6 * rn + r))
    else:
        col_ptr, row_idx, blk_src = (np.asarray(plan_arrays[k]) for k in ("col_ptr", "row_idx", "blk_src"))
        for j in range(n):
            for b in range(int(col_ptr[j]), int(col_ptr[j + 1])):
                if int(row_idx[b]) == j:
                    continue
                src = int(blk_src[b])
                rn, cn, tr = src >> 9, (src >> 1) & 255, src & 1
                fr, fc = b % 6, (b // 6 + b) % 6                     # the element of the factor's block; S stores it transposed if tr
                r, c = (fc, fr) if tr else (fr, fc)
                out.append(Fault("nan_off", (6 * rn + r) * D + 6 * cn + c, float("nan"), 1, 6 * rn + r))
    for k in range(D):
        out.append(Fault("nan_y", D * D + k, float("nan"), 2, k))
    return out


def oracle_step(d, fixedp, weights=None, **kw):
    return oracle.ba_step(d["poses"], d["patches"], d["mono"], d["intrinsics"], d["targets3"],
                          d["weights_pose"] if weights is None else weights, d["ii"], d["jj"], d["kk"], d["bounds"],
                          fixedp=fixedp, want_system=True, **kw)


def localised_failure(d, p, fixedp=1):
    """A real problem whose only failing pivot is free pose p (frame fixedp + p): the pose weights of every edge that touches the
    frame are zero, so its block of S is exactly 0, and ep is negative but six orders below the other poses' diagonals.
    -> (weights_pose, ep)"""
    f = int(fixedp) + int(p)
    w = np.array(d["weights_pose"], np.float64, copy=True)
    w[(np.asarray(d["ii"]) == f) | (np.asarray(d["jj"]) == f)] = 0.0
    S = oracle_step(d, fixedp, weights=w)["S"]
    dg = np.diag(S).reshape(-1, 6)
    others = np.delete(dg, p, axis=0)
    ep = -1e-6 * float(others.min())
    return w, float(np.float32(ep))             # (the ABI's ep is a float32: what the kernels and the oracle both get)
