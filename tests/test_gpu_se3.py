"""-m gpu: the element-wise SE3 HIP kernels (include/batrack_se3.h, row f-1 of SURVEY.md §8)
against the float64 torch formulas of oracle/se3_torch.py on the CPU, plus the identities of the
reference's own test script (lietorch/run_tests.py:16-52) evaluated on the device."""
import numpy as np
import pytest
import torch

from batrack_amd.backend import lietorch_backends as lb
from batrack_amd.backend.lietorch import SE3
from oracle.se3_torch import SE3Ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.manual_seed(1)


def cpu64(x):
    return x.detach().cpu().double()


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-6), (torch.float64, 1e-12)])
def test_ops_match_cpu_float64(dtype, tol):
    B = 4099
    a = (0.7 * torch.randn(B, 6, dtype=torch.float64)).to(dtype)
    a[:5] *= 1e-8                                            # small-angle branch
    X = SE3Ref.exp(cpu64(a))
    Y = SE3Ref.exp(0.5 * torch.randn(B, 6, dtype=torch.float64))
    p4 = torch.randn(B, 4, dtype=torch.float64)
    v6 = torch.randn(B, 6, dtype=torch.float64)
    g = lambda t: t.to(dtype).to(DEV).contiguous()
    Xg, Yg = g(X.data), g(Y.data)
    Xr, Yr = SE3Ref(cpu64(Xg)), SE3Ref(cpu64(Yg))                 # reference on the same rounded inputs
    rel = lambda got, ref: float((cpu64(got) - ref).norm() / ref.norm())
    assert rel(lb.expm(3, g(a)), SE3Ref.exp(cpu64(g(a))).data) < tol
    assert rel(lb.inv(3, Xg), Xr.inv().data) < tol
    assert rel(lb.mul(3, Xg, Yg), (Xr * Yr).data) < tol
    assert rel(lb.act4(3, Xg, g(p4)), Xr.act(cpu64(g(p4)))) < tol
    assert rel(lb.act(3, Xg, g(p4[:, :3])), Xr.act(cpu64(g(p4[:, :3])))) < tol
    assert rel(lb.adjT(3, Xg, g(v6)), Xr.adjT(cpu64(g(v6)))) < tol
    assert rel(lb.as_matrix(3, Xg), Xr.matrix()) < tol
    assert rel(lb.logm(3, Xg), Xr.log()) < (5e-5 if dtype == torch.float32 else 1e-9)
    # adj is the transpose-adjoint's adjoint: <Ad a, b> == <a, Ad^T b>
    b6 = torch.randn(B, 6, dtype=torch.float64)
    lhs = (cpu64(lb.adj(3, Xg, g(v6))) * cpu64(g(b6))).sum(-1)
    rhs = (cpu64(g(v6)) * cpu64(lb.adjT(3, Xg, g(b6)))).sum(-1)
    assert float((lhs - rhs).abs().max()) < (2e-4 if dtype == torch.float32 else 1e-10)


def test_reference_identities_on_device():
    B = 1000
    a = 0.5 * torch.randn(B, 6, dtype=torch.float64, device=DEV)
    X = SE3.exp(a)                                                        # HIP path (GPU tensor)
    assert torch.allclose(X.log(), a, atol=1e-8)                          # Log(Exp(a)) == a
    I = (X * X.inv()).data
    ref = torch.zeros_like(I); ref[:, 6] = 1
    assert torch.allclose(I, ref, atol=1e-8)                              # X X^-1 == identity
    b = 0.3 * torch.randn(B, 6, dtype=torch.float64, device=DEV)
    lhs = (X * SE3.exp(b)).data
    rhs = (SE3.exp(lb.adj(3, X.data, b)) * X).data                        # X Exp(b) == Exp(Ad_X b) X
    sign = torch.sign((lhs[:, 3:] * rhs[:, 3:]).sum(-1, keepdim=True))
    assert torch.allclose(lhs[:, :3], rhs[:, :3], atol=1e-8) and torch.allclose(lhs[:, 3:], sign * rhs[:, 3:], atol=1e-8)
    p = torch.randn(B, 4, dtype=torch.float64, device=DEV)
    assert torch.allclose(X.act(p), torch.einsum("bij,bj->bi", lb.as_matrix(3, X.data), p), atol=1e-8)


def test_wrapper_broadcasts_like_the_reference():
    """poses[:, jj] * poses[:, ii].inv(), Gij[:, :, None, None] * X0 (projective_ops.py:61-66)."""
    P = SE3.exp(0.3 * torch.randn(1, 12, 6, device=DEV))
    ii = torch.randint(0, 12, (40,), device=DEV); jj = torch.randint(0, 12, (40,), device=DEV)
    Gij = P[:, jj] * P[:, ii].inv()
    X0 = torch.randn(1, 40, 3, 3, 4, device=DEV)
    X1 = Gij[:, :, None, None] * X0
    assert tuple(X1.shape) == (1, 40, 3, 3, 4)
    Pc = SE3Ref(P.data.cpu().double())
    Gc = Pc[:, jj.cpu()] * Pc[:, ii.cpu()].inv()
    X1c = Gc[:, :, None, None] * X0.cpu().double()
    assert float((X1.cpu().double() - X1c).abs().max()) < 2e-5
    M = Gij.matrix()
    assert tuple(M.shape) == (1, 40, 4, 4)


def test_rejects_other_groups_and_cpu_tensors():
    x = torch.zeros(4, 7, device=DEV); x[:, 6] = 1
    with pytest.raises(NotImplementedError):
        lb.inv(4, x)                                         # Sim3
    with pytest.raises(RuntimeError):
        lb.inv(3, x.cpu())
    with pytest.raises(NotImplementedError):
        lb.inv_backward(3, x, x)
    with pytest.raises(RuntimeError):
        SE3(x.cpu()).inv()                                   # the wrapper has no host path either
    with pytest.raises(RuntimeError):
        SE3.exp(torch.zeros(2, 6))


# ------------------------------------------------------------------ past one grid pass, every branch of Exp and Log
DT = [(torch.float32, 2e-6, 1e-5), (torch.float64, 1e-12, 1e-12)]          # dtype, whole-array gate (as above), per-row gate


def _rowerr(got, ref):
    """Per row: the largest error relative to 1 + the row's largest entry."""
    got, ref = cpu64(got).reshape(len(ref), -1), ref.reshape(len(ref), -1)
    return (got - ref).abs().amax(-1) / (1 + ref.abs().amax(-1))


@pytest.mark.parametrize("dtype,tol,rtol", DT)
def test_every_row_of_a_three_pass_grid(dtype, tol, rtol):
    """The launches cap the grid at 4096 x 256 threads and stride over the rest: B = 2 * 4096 * 256 + 37 runs the loop three
    times, the last pass partial.  Every row of all nine ops against oracle/se3_torch.py on the same rounded inputs."""
    B = 4096 * 256 * 2 + 37
    gen = torch.Generator().manual_seed(11)
    a = 0.7 * torch.randn(B, 6, dtype=torch.float64, generator=gen)
    nrm = a[:, 3:].norm(dim=1, keepdim=True)
    a[:, 3:] *= torch.clamp(3.0 / nrm, max=1.0)                               # angles below pi: Log is then Exp's inverse
    g = lambda t: t.to(dtype).to(DEV).contiguous()
    ag = g(a)
    Xg, Yg = g(SE3Ref.exp(cpu64(ag)).data), g(SE3Ref.exp(0.5 * torch.randn(B, 6, dtype=torch.float64, generator=gen)).data)
    Xr, Yr = SE3Ref(cpu64(Xg)), SE3Ref(cpu64(Yg))
    p4, v6, b6 = (g(torch.randn(B, k, dtype=torch.float64, generator=gen)) for k in (4, 6, 6))
    checks = {"exp": (lb.expm(3, ag), SE3Ref.exp(cpu64(ag)).data), "inv": (lb.inv(3, Xg), Xr.inv().data),
              "mul": (lb.mul(3, Xg, Yg), (Xr * Yr).data), "act4": (lb.act4(3, Xg, p4), Xr.act(cpu64(p4))),
              "act": (lb.act(3, Xg, p4[:, :3].contiguous()), Xr.act(cpu64(p4[:, :3]))), "adjT": (lb.adjT(3, Xg, v6), Xr.adjT(cpu64(v6))),
              "matrix": (lb.as_matrix(3, Xg), Xr.matrix()), "log": (lb.logm(3, Xg), Xr.log())}
    for name, (got, ref) in checks.items():
        assert tuple(got.shape)[0] == B
        lt = 5e-5 if (name == "log" and dtype == torch.float32) else (1e-9 if name == "log" else tol)
        assert float((cpu64(got) - ref).norm() / ref.norm()) < lt, name
        e = _rowerr(got, ref)
        bad = torch.nonzero(e > (50 * rtol if name == "log" else rtol)).flatten()
        assert bad.numel() == 0, (name, bad[:8].tolist(), float(e.max()))
    # adj (no oracle of its own): <Ad a, b> == <a, Ad^T b> on every row
    lhs = (cpu64(lb.adj(3, Xg, v6)) * cpu64(b6)).sum(-1)
    rhs = (cpu64(v6) * cpu64(lb.adjT(3, Xg, b6))).sum(-1)
    e = (lhs - rhs).abs() / (1 + lhs.abs())
    assert float(e.max()) < (1e-4 if dtype == torch.float32 else 1e-10), int(e.argmax())


def _exp_mp(a):
    """Exp of one tangent (tau, phi) with mpmath at 60 digits: (t, q) as float64."""
    import mpmath as mp
    mp.mp.dps = 60
    tau, phi = [mp.mpf(float(x)) for x in a[:3]], [mp.mpf(float(x)) for x in a[3:]]
    th = mp.sqrt(sum(p * p for p in phi))
    cross = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    if th == 0:
        return [float(x) for x in tau] + [0.0, 0.0, 0.0, 1.0]
    p1 = cross(phi, tau)
    p2 = cross(phi, p1)
    c1, c2 = (1 - mp.cos(th)) / th ** 2, (th - mp.sin(th)) / th ** 3
    t = [tau[c] + c1 * p1[c] + c2 * p2[c] for c in range(3)]
    q = [phi[c] / th * mp.sin(th / 2) for c in range(3)] + [mp.cos(th / 2)]
    return [float(x) for x in t + q]


EXP_ANGLES = [0.0, 1e-9, 0.999e-6, 1.001e-6, 1e-3, 0.2499, 0.2501, 1.0, np.pi - 1e-4, np.pi, np.pi + 1e-3, 2 * np.pi - 1e-3, 3 * np.pi]


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-6), (torch.float64, 1e-13)])
def test_exp_at_every_branch_switch_vs_mpmath(dtype, tol):
    """Exp's series below 1e-6, its c2 series below 0.25, angles up to and past pi and 2 pi, against mpmath on the rounded
    inputs: the rotation as a quaternion up to sign, the translation relative to 1 + |tau|."""
    rng = np.random.default_rng(5)
    rows = []
    for th in EXP_ANGLES:
        for _ in range(6):
            ax = rng.standard_normal(3)
            rows.append(np.concatenate([rng.standard_normal(3), th * ax / np.linalg.norm(ax)]))
    a = torch.as_tensor(np.array(rows)).to(dtype)
    got = cpu64(lb.expm(3, a.to(DEV).contiguous())).numpy()
    ref = np.array([_exp_mp(r) for r in cpu64(a).numpy()])
    s = np.sign((got[:, 3:] * ref[:, 3:]).sum(-1, keepdims=True))
    eq = np.abs(got[:, 3:] - s * ref[:, 3:]).max(-1)
    et = np.abs(got[:, :3] - ref[:, :3]).max(-1) / (1 + np.abs(ref[:, :3]).max(-1))
    th = np.repeat(EXP_ANGLES, 6)
    assert eq.max() < tol, (th[eq.argmax()], eq.max())
    assert et.max() < 2 * tol, (th[et.argmax()], et.max())


def _log_cases(rng):
    """Stored quaternions at every branch of so3.h:115-151's Log: (qx qy qz qw) before normalisation."""
    def q(n, w):
        ax = rng.standard_normal(3)
        return np.concatenate([n * ax / np.linalg.norm(ax), [w]])
    out = []
    for w in (-0.9, -0.3, -1e-3):                                              # w < 0 (angles past pi)
        out.append(q(np.sqrt(1 - w * w), w))
    for w in (5e-7, -5e-7, 9.9e-7, -9.9e-7, 1.1e-6, -1.1e-6, 0.0, -0.0):       # |w| < 1e-6 on both sides of zero, w == 0, just outside
        out.append(q(np.sqrt(1 - w * w), w))
    for n in (0.0, 1e-9, 0.9e-6, 1.1e-6, 1e-4):                                # |imag|^2 below and above 1e-12
        for w in (1.0, -1.0):
            out.append(q(n, w))
    for scale in (1e-3, 1e3):                                                  # normalised on load
        for v in list(out[:4]) + [q(0.6, 0.8), q(0.8, -0.6)]:
            out.append(scale * v)
    return np.array(out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_log_at_every_branch(dtype):
    """Log against oracle/se3_torch.py (the branch rule of so3.h:115-151 restated) on the same rounded inputs; |phi| <= pi;
    Exp(Log(X)) == X up to the quaternion's sign (the |w| < 1e-6 branch rounds the angle to pi: off by |w| there)."""
    rng = np.random.default_rng(9)
    Q = _log_cases(rng)
    X = np.concatenate([rng.standard_normal((len(Q), 3)), Q], 1)
    Xg = torch.as_tensor(X).to(dtype).to(DEV).contiguous()
    got = cpu64(lb.logm(3, Xg))
    ref = SE3Ref(cpu64(Xg)).log()
    f32 = dtype == torch.float32
    e = (got - ref).abs().amax(-1) / (1 + ref.abs().amax(-1))
    assert float(e.max()) < (2e-5 if f32 else 1e-12), (int(e.argmax()), float(e.max()))
    assert float(got[:, 3:].norm(dim=-1).max()) <= np.pi * (1 + (1e-6 if f32 else 1e-15))
    back = cpu64(lb.expm(3, lb.logm(3, Xg)))
    qn = cpu64(Xg)[:, 3:] / cpu64(Xg)[:, 3:].norm(dim=-1, keepdim=True)
    s = torch.sign((back[:, 3:] * qn).sum(-1, keepdim=True))
    s[s == 0] = 1
    w = qn[:, 3].abs()
    slack = torch.where(w < 1e-6, w, torch.zeros_like(w)) + (2e-6 if f32 else 1e-12)
    assert bool(((back[:, 3:] - s * qn).abs().amax(-1) <= slack).all()), float(((back[:, 3:] - s * qn).abs().amax(-1) - slack).max())
    assert float((back[:, :3] - cpu64(Xg)[:, :3]).abs().max()) < (1e-4 if f32 else 1e-9)
