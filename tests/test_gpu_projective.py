"""bt_reproject (include/batrack_projective.h, row f-3): the fused reprojection against the reference's golden
coordinates (float64 run of its transform), against the oracle's per-edge coordinates, and against the composed
tensor operations it replaces — patch sizes 1 and 3, depth / valid / translation-only variants, bad indices."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
from batrack_amd import _lib, graphgen
from batrack_amd.backend import projective_ops as pops
from batrack_amd.backend.lietorch import SE3

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"


def gpu_inputs(poses, patches, intr, ii, jj, kk, p=1, seed=0):
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=DEV)
    pat = f32(patches)[None, :, :, None, None]
    if p > 1:                                          # a p x p window around the centre, as patchify makes it
        rng = np.random.default_rng(seed)
        off = torch.as_tensor(rng.normal(0, 1.5, (1, pat.shape[1], 3, p, p)).astype(np.float32), device=DEV)
        off[:, :, 2] = 0.0
        off[:, :, :, p // 2, p // 2] = 0.0
        pat = pat + off
    return (SE3(f32(poses)[None]), pat.contiguous(), f32(intr)[None],
            *(torch.as_tensor(np.asarray(a, np.int64), device=DEV) for a in (ii, jj, kk)))


@pytest.mark.parametrize("name", ["c1", "c1_rough", "window_small"])
def test_fused_matches_reference_coordinates(name):
    d = dict(np.load(os.path.join(GOLD, name + ".npz")))
    G, pat, K, ii, jj, kk = gpu_inputs(d["poses"], d["patches"], d["intrinsics"], d["ii"], d["jj"], d["kk"])
    x, v = pops.transform(G, pat, K, ii, jj, kk, valid=True)
    assert x.shape == (1, ii.numel(), 1, 1, 2) and v.shape == (1, ii.numel(), 1, 1)
    o = oracle.edges(d["poses"], d["patches"], d["intrinsics"], d["targets3"], d["weights"], d["ii"], d["jj"], d["kk"], d["bounds"])
    got = x[0, :, 0, 0].cpu().numpy().astype(np.float64)
    # float32 against float64: relative to the pixel magnitude; points near the camera plane (rough graphs) are
    # amplified by 1/Z and compared where the reference itself is tame
    def close(ref):
        tame = np.isfinite(ref).all(1) & (np.abs(ref).max(1) < 1e4)
        assert tame.mean() > 0.9
        return (np.abs(got - ref) / (100.0 + np.abs(ref)))[tame].max()         # 2e-3 px at the image centre scale
    if "tf64.coords" in d:
        assert close(d["tf64.coords"]) < 2e-5
        flips = v[0, :, 0, 0].cpu().numpy() != d["tf64.valid"].astype(np.float32)
        assert flips.mean() < 1e-3
    assert close(o["coords"]) < 2e-5


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("depth,tonly", [(False, False), (True, False), (False, True), (True, True)])
def test_fused_equals_composed_operations(p, depth, tonly):
    g = graphgen.make_random_graph(20, 64, seed=5)
    G, pat, K, ii, jj, kk = gpu_inputs(g.poses, g.patches, g.intrinsics, g.ii, g.jj, g.kk, p=p)
    a, va = pops.transform(G, pat, K, ii, jj, kk, depth=depth, valid=True, tonly=tonly)
    b, vb = pops.transform(G, pat, K, ii, jj, kk, depth=depth, valid=True, tonly=tonly, fused=False)
    assert a.shape == b.shape == (1, ii.numel(), p, p, 3 if depth else 2) and va.shape == vb.shape
    # points close to the camera plane amplify rounding by 1/Z: compare where the composed result is tame
    tame = (b[..., :2].abs().amax(-1) < 1e4)
    assert tame.float().mean() > 0.9
    err = ((a - b).abs() / (100.0 + b.abs()))[tame]
    assert float(err.max()) < 2e-5, float(err.max())
    assert float((va != vb).float().mean()) < 1e-3            # Z within rounding of 0.2 may flip
    # non-contiguous index views and a strided patch tensor are accepted
    a2 = pops.transform(G, pat.expand(1, -1, -1, -1, -1), K, ii[::2], jj[::2], kk[::2], depth=depth, tonly=tonly)
    assert torch.equal(a2, a[:, ::2])


def test_flow_mag_and_self_reprojection():
    g = graphgen.make_config("C1", seed=0)
    G, pat, K, ii, jj, kk = gpu_inputs(g.poses, g.patches, g.intrinsics, g.ii, g.jj, g.kk)
    same = pops.transform(G, pat, K, ii, ii, kk)
    assert float((same[0, :, 0, 0] - pat[0, kk, :2, 0, 0]).abs().max()) < 1e-3
    f = pops.flow_mag(G, pat, K, ii, jj, kk, beta=0.5)
    c0 = pops.transform(G, pat, K, ii, ii, kk, fused=False)
    c1 = pops.transform(G, pat, K, ii, jj, kk, fused=False)
    c2 = pops.transform(G, pat, K, ii, jj, kk, tonly=True, fused=False)
    ref = 0.5 * (c1 - c0).norm(dim=-1) + 0.5 * (c2 - c0).norm(dim=-1)
    assert float((f - ref).abs().max()) < 1e-2 and f.shape == ref.shape


def test_abi_rejects_and_flags():
    L = _lib.lib()
    g = graphgen.make_config("C1", seed=0)
    G, pat, K, ii, jj, kk = gpu_inputs(g.poses, g.patches, g.intrinsics, g.ii, g.jj, g.kk)
    E = ii.numel()
    out = torch.zeros(E, 2, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    args = lambda **k: [k.get("poses", G.data.data_ptr()), G.data.shape[1], pat.data_ptr(), pat.shape[1], k.get("pe", 1), K.data_ptr(),
                        ii.data_ptr(), jj.data_ptr(), kk.data_ptr(), k.get("E", E), k.get("mode", 0), out.data_ptr(), None, st]
    assert L.bt_reproject(*args(E=-1)) == _lib.BT_EINVAL
    assert L.bt_reproject(*args(pe=0)) == _lib.BT_EINVAL
    assert L.bt_reproject(*args(mode=7)) == _lib.BT_EINVAL
    assert L.bt_reproject(*args(poses=None)) == _lib.BT_EINVAL
    assert L.bt_reproject(*args(E=0)) == _lib.BT_OK
    bad = jj.clone(); bad[3] = 10 ** 6; bad[5] = -1
    x, v = pops.transform(G, pat, K, ii, bad, kk, valid=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(x[0, 3]).all()) and bool(torch.isnan(x[0, 5]).all()) and float(v[0, 3].sum() + v[0, 5].sum()) == 0.0
    good = torch.ones(E, dtype=torch.bool, device=DEV); good[3] = good[5] = False
    assert not bool(torch.isnan(x[0, good]).any())


# ------------------------------------------------------------------ past one grid pass, at the argument limits
def _qrot64(q, v):
    qv, w = q[..., :3], q[..., 3:]
    uv = 2.0 * np.cross(qv, v)
    return v + w * uv + np.cross(qv, uv)


def reproject64(poses, patches, intr, ii, jj, kk, p, tonly=False):
    """projective_ops.transform (iproj -> G_j G_i^-1 -> act4 -> proj, projective_ops.py:19-75) in float64 on the CPU for
    edges ii, jj, kk: (u, v, projected inverse depth, Z) per patch pixel, [E, p*p, 4]."""
    pat = patches.reshape(len(patches), 3, p * p).astype(np.float64)[kk]                 # [E,3,pe]
    q = poses[:, 3:].astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    t = poses[:, :3].astype(np.float64)
    Ki, Kj = intr[ii].astype(np.float64)[:, :, None], intr[jj].astype(np.float64)[:, :, None]
    X0 = np.stack([(pat[:, 0] - Ki[:, 2]) / Ki[:, 0], (pat[:, 1] - Ki[:, 3]) / Ki[:, 1], np.ones_like(pat[:, 0])], -1)  # [E,pe,3]
    d = pat[:, 2]
    qiv = np.concatenate([-q[ii, :3], q[ii, 3:]], 1)
    tij = t[jj] + _qrot64(q[jj], -_qrot64(qiv, t[ii]))                                   # t_j - R_j R_i^T t_i
    R = X0 if tonly else _qrot64(q[jj][:, None], _qrot64(qiv[:, None], X0))
    X1 = R + tij[:, None] * d[..., None]
    iz = 1.0 / np.maximum(X1[..., 2], 1e-2)
    return np.stack([Kj[:, 0] * iz * X1[..., 0] + Kj[:, 2], Kj[:, 1] * iz * X1[..., 1] + Kj[:, 3], iz * d, X1[..., 2]], -1)


def _reproject_raw(poses, patches, intr, ii, jj, kk, pe, mode, E=None):
    """bt_reproject into NaN-filled outputs: (status, coords, valid)."""
    L = _lib.lib()
    E = ii.numel() if E is None else E
    no = 3 if mode & 1 else 2
    coords = torch.full((max(E, 1) * pe, no), float("nan"), device=DEV)
    valid = torch.full((max(E, 1) * pe,), float("nan"), device=DEV)
    rc = L.bt_reproject(poses.data_ptr(), poses.shape[0], patches.data_ptr(), patches.shape[0], pe, intr.data_ptr(), ii.data_ptr(),
                        jj.data_ptr(), kk.data_ptr(), E, mode, coords.data_ptr(), valid.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, coords, valid


def _random_problem(E, p, n_poses, n_patches, seed):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n_poses, 4)) * 0.1 + np.array([0, 0, 0, 1.0])
    poses = np.concatenate([rng.standard_normal((n_poses, 3)) * 0.3, q * rng.uniform(0.5, 2.0, (n_poses, 1))], 1).astype(np.float32)
    intr = np.tile(np.array([320.0, 310.0, 160.0, 120.0], np.float32), (n_poses, 1))
    patches = np.empty((n_patches, 3, p, p), np.float32)
    patches[:, 0] = rng.uniform(0, 320, (n_patches, 1, 1)) + rng.normal(0, 1.5, (n_patches, p, p))
    patches[:, 1] = rng.uniform(0, 240, (n_patches, 1, 1)) + rng.normal(0, 1.5, (n_patches, p, p))
    patches[:, 2] = rng.uniform(0.05, 1.0, (n_patches, 1, 1))
    idx = lambda n: rng.integers(0, n, E).astype(np.int64)
    ii, jj, kk = idx(n_poses), idx(n_poses), idx(n_patches)
    return poses, patches, intr, ii, jj, kk


@pytest.mark.parametrize("E,p,mode", [(600_000, 3, 1), (600_000, 3, 2), (4_300_000, 1, 1)])
def test_reproject_past_one_grid_pass(E, p, mode):
    """The launch caps the grid at 16384 x 256 threads and strides over the rest: E * patch_elems of 5.4M and 4.3M.  Every
    output written (NaN-filled beforehand), indices n - 1 (valid) and n (NaN, invalid) planted at the tail too, and a
    subsample of 20k edges that includes the last ones against the float64 restatement."""
    n_poses, n_patches = 40, 3000
    poses, patches, intr, ii, jj, kk = _random_problem(E, p, n_poses, n_patches, seed=E + p)
    ii[-3], jj[-3], kk[-3] = n_poses - 1, n_poses - 1, n_patches - 1                    # last valid index of each kind
    ii[-5], jj[-4], kk[-2] = n_poses, n_poses, n_patches                                # one past each
    ii[7], kk[8] = n_poses, n_patches
    bad = np.zeros(E, bool)
    bad[[-5, -4, -2, 7, 8]] = True
    g = lambda a: torch.as_tensor(a, device=DEV).contiguous()
    rc, coords, valid = _reproject_raw(g(poses), g(patches), g(intr), g(ii), g(jj), g(kk), p * p, mode)
    assert rc == _lib.BT_OK
    pe = p * p
    c = coords.view(E, pe, -1).cpu().numpy().astype(np.float64)
    v = valid.view(E, pe).cpu().numpy()
    assert np.isnan(c[bad]).all() and (v[bad] == 0).all()
    assert not np.isnan(c[~bad]).any() and np.isin(v[~bad], [0.0, 1.0]).all()
    rng = np.random.default_rng(1)
    sub = np.unique(np.concatenate([rng.choice(E, 20000, replace=False), np.arange(E - 2000, E)]))
    sub = sub[~bad[sub]]
    ref = reproject64(poses, patches, intr, ii[sub], jj[sub], kk[sub], p, tonly=bool(mode & 2))
    got = c[sub]
    tame = np.abs(ref[..., :2]).max(-1) < 1e4
    assert tame.mean() > 0.9 and tame[-100:].any()
    err = np.abs(got - ref[..., :got.shape[-1]]) / (100.0 + np.abs(ref[..., :got.shape[-1]]))
    assert err[tame].max() < 2e-5, err[tame].max()
    clear = np.abs(ref[..., 3] - 0.2) > 1e-4                                            # Z within rounding of 0.2 may flip
    assert np.array_equal(v[sub][clear], (ref[..., 3] > 0.2)[clear].astype(np.float32))


def test_reproject_largest_patch():
    """patch_elems = 4096 (64 x 64 patches) accepted and right against the float64 restatement; 4097 refused before any launch
    (the NaN-filled outputs stay untouched)."""
    p, E = 64, 300
    poses, patches, intr, ii, jj, kk = _random_problem(E, p, 12, 50, seed=64)
    g = lambda a: torch.as_tensor(a, device=DEV).contiguous()
    args = (g(poses), g(patches), g(intr), g(ii), g(jj), g(kk))
    rc, coords, valid = _reproject_raw(*args, 4096, 1)
    assert rc == _lib.BT_OK
    ref = reproject64(poses, patches, intr, ii, jj, kk, p)
    got = coords.view(E, 4096, 3).cpu().numpy().astype(np.float64)
    tame = np.abs(ref[..., :2]).max(-1) < 1e4
    assert tame.mean() > 0.9
    assert (np.abs(got - ref[..., :3]) / (100.0 + np.abs(ref[..., :3])))[tame].max() < 2e-5
    # (patches 0..39 only and E * 4096 // 4097 edges: even a launch would stay inside every buffer)
    rc, coords, valid = _reproject_raw(*args[:5], g(kk % 40), 4097, 1, E=E * 4096 // 4097)
    assert rc == _lib.BT_EINVAL
    assert bool(torch.isnan(coords).all()) and bool(torch.isnan(valid).all())
