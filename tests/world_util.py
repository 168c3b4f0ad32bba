"""The specification of bt_world_tracks (include/batrack_projective.h) restated in numpy, in the dtype of its inputs:
what tests/golden/world_tracks.npz (made by the unmodified reference) is compared with on the CPU, and the helpers the
GPU tests share.  Written from the header's formulas, not from the reference's program text."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "world_tracks.npz")
CASES = ("a", "b", "c")
CLAMP = 1e-2


def qrot(q, v):
    """Rotate v by the unit quaternion q = (x, y, z, w)."""
    qv, w = q[..., :3], q[..., 3:]
    uv = 2.0 * np.cross(qv, v)
    return v + w * uv + np.cross(qv, uv)


def unit(q):
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def inv_act4(t, q, X, d):
    """G^-1 * (X, d) = (R^T (X - t d), d) -> the first three components."""
    qi = np.concatenate([-q[..., :3], q[..., 3:]], -1)
    return qrot(qi, X - t * d)


def np_world_tracks(poses, intrinsics, patches, ix, patches_local, local_weights, m):
    """Returns (points [m,3], world [NM,S,3], patches_local_out [NM,S,3], Xc3 [m,S]); rows past m of `world` are zero and of
    `patches_local_out` the input.  Xc3 is the third component of G_j * Pw (what the 1e-2 clamp looks at)."""
    dt = poses.dtype
    N, (NM, S) = poses.shape[0], patches_local.shape[:2]
    mid = (S + 1) // 2 - 1
    t, q = poses[:, :3], unit(poses[:, 3:])
    pe = patches.reshape(NM, 3, -1)
    p = int(round(np.sqrt(pe.shape[-1])))
    c = (p // 2) * (p + 1)
    i = ix[:m]
    with np.errstate(all="ignore"):
        x, y, d = pe[:m, 0, c], pe[:m, 1, c], pe[:m, 2, c]
        K = intrinsics[i]
        X0 = np.stack([(x - K[:, 2]) / K[:, 0], (y - K[:, 3]) / K[:, 1], np.ones_like(x)], -1)
        Pw = inv_act4(t[i], q[i], X0, d[:, None])                                       # [m,3]
        points = Pw / d[:, None]
        live = local_weights.reshape(NM, S)[:m].sum(1) > 0
        j = np.clip(i[:, None] + np.arange(S)[None] - mid, 0, N - 1)                    # [m,S]
        Kj = intrinsics[j]
        # live: the world point, re-projected
        Xc = qrot(q[j], np.broadcast_to(Pw[:, None], (m, S, 3))) + t[j] * d[:, None, None]
        r = 1.0 / np.maximum(Xc[..., 2], dt.type(CLAMP))
        proj = np.stack([Kj[..., 0] * (r * Xc[..., 0]) + Kj[..., 2], Kj[..., 1] * (r * Xc[..., 1]) + Kj[..., 3], r * d[:, None]], -1)
        # not live: the tracker's (u, v, e) back-projected in every window frame
        u, v, e = (patches_local[:m, :, k] for k in range(3))
        Xd = np.stack([(u - Kj[..., 2]) / Kj[..., 0], (v - Kj[..., 3]) / Kj[..., 1], np.ones_like(u)], -1)
        Wd = inv_act4(t[j], q[j], Xd, e[..., None]) / e[..., None]
    world = np.zeros((NM, S, 3), dt)
    world[:m] = np.where(live[:, None, None], points[:, None], Wd)
    out = patches_local.copy()
    out[:m] = np.where(live[:, None, None], proj, patches_local[:m])
    return points, world, out, Xc[..., 2]


def load_case(D, c, dtype=np.float64):
    """Inputs of fixture case `c` in `dtype`, as np_world_tracks takes them (and m)."""
    f = lambda k: D[f"{c}.{k}"].astype(dtype)
    return (f("poses"), f("intrinsics"), f("patches"), D[f"{c}.ix"].astype(np.int64), f("patches_local"), f("local_weights"),
            int(D[f"{c}.m"]))


def rel_err(got, ref):
    """max |got - ref| / (1 + |ref|) over the finite entries of ref: the fixture's `gate.*` measure."""
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok].astype(np.float64) - ref[ok]) / (1.0 + np.abs(ref[ok]))).max())


def uv_err(got, ref):
    """The project's gate for fused reprojection (tests/test_gpu_projective.py:45-49): |got - ref| / (100 + |ref|) over
    the entries with |ref| < 1e4; returns (largest value, share of entries compared)."""
    tame = np.isfinite(ref) & (np.abs(ref) < 1e4)
    if not tame.any():
        return 0.0, 0.0
    return float((np.abs(got[tame].astype(np.float64) - ref[tame]) / (100.0 + np.abs(ref[tame]))).max()), float(tame.mean())


def random_inputs(N, M, S_slam, n, seed, live_frac=0.7, S_local=None, p=None):
    """Seeded float32 inputs at a user's size, numpy.  The camera circles (radius 0.3, 0.02 a frame) and sways in front of
    the scene through the whole buffer, disparities in [0.2, 1]: |t| <= 0.7 and |t| / d <= 3.5 as in fixture case (a).  The
    rounding of a float32 evaluation is a few ulp of the intermediate magnitudes |t|, |t| / d, which the measure
    |err| / (1 + |ref|) does not scale with, so the fixture's e32 carries over to these sizes only at the conditioning it was
    measured at (measured on the GPU: with the camera 4 units from the origin the older composed operations themselves are
    2.8e-6 from a float64 evaluation, 30 x e32).  Tracks lie in front of every camera of their window (camera-frame depth
    > 0.5, away from the 1e-2 clamp), about `live_frac` of them are live, a quarter of the other tracks' slots were never
    filled.  `S_local`: any window length in place of 2 * S_slam - 1, even ones included.  `p`: p x p patches whose centre pixel
    (p/2, p/2) is the track and whose every other pixel is a decoy in +-1000 (a wrong centre index or plane stride moves the
    result by far more than any gate); drawn after everything else, so that the other arrays do not depend on it.  Returns
    a dict with the arguments of the C entry point and m = n * M."""
    rng = np.random.default_rng(seed)
    S, NM = (2 * S_slam - 1 if S_local is None else int(S_local)), N * M
    s = np.arange(N)[:, None]
    th = s / 15.0                                                                       # a circle of radius 0.3: 0.02 a frame
    centre = np.concatenate([0.3 * np.sin(th), 0.05 * np.sin(0.7 * s), 0.3 * (1.0 - np.cos(th))], 1)
    ang = 0.5 * (0.1 * np.sin(0.05 * s) + 0.02 * np.sin(0.3 * s))                       # the camera sways, facing the scene
    q = np.concatenate([np.sin(ang) * np.array([0.02, -0.9995, 0.02]), np.cos(ang)], 1)
    t = -qrot(unit(q), centre)                                                          # world -> camera
    q = q * rng.uniform(0.7, 1.4, (N, 1))
    K = np.array([320.0, 310.0, 160.0, 120.0]) * rng.uniform(0.9, 1.1, (N, 4))
    patches = np.stack([rng.uniform(10, 310, NM), rng.uniform(10, 230, NM), rng.uniform(0.2, 1.0, NM)], 1)
    pl = np.stack([rng.uniform(0, 320, (NM, S)), rng.uniform(0, 240, (NM, S)), rng.uniform(0.2, 1.0, (NM, S))], -1)
    live = rng.random(NM) < live_frac
    w = rng.uniform(0.1, 1.0, (NM, S)) * (rng.random((NM, S)) < 0.6)
    w[live, (S + 1) // 2 - 1] = 0.5
    w[~live] = 0.0
    pl[(rng.random((NM, S)) < 0.25) & ~live[:, None]] = 0.0
    f = lambda a: np.ascontiguousarray(a, np.float32)
    patches = patches.reshape(NM, 3, 1, 1)
    if p is not None:
        track = patches[..., 0, 0]
        patches = rng.uniform(-1000.0, 1000.0, (NM, 3, p, p))
        patches[:, :, p // 2, p // 2] = track
    return dict(poses=f(np.concatenate([t, q], 1)), intrinsics=f(K), patches=f(patches),
                ix=(np.arange(NM) // M).astype(np.int64), patches_local=f(pl), local_weights=f(w), m=n * M)


def composed_world_tracks(SE3, poses, patches, intrinsics, ix, patches_local, local_weights, m):
    """The specification composed from the operations the package had before the fused kernel — pops.point_cloud,
    pops.proj(depth=True) and the SE3 gather / inverse / action kernels — on GPU tensors: poses [1,N,7], patches
    [1,NM,3,p,p], intrinsics [1,N,4], ix [>= m], patches_local [1,NM,S,3] (not modified), local_weights with NM*S elements.
    Returns (points [m,3], world [1,NM,S,3] with zeros past m, patches_local_out [1,NM,S,3])."""
    import torch
    from batrack_amd.backend import projective_ops as pops
    G = SE3(poses)
    N, NM, S = poses.shape[1], patches_local.shape[1], patches_local.shape[2]
    mid, c = (S + 1) // 2 - 1, patches.shape[-1] // 2
    i = ix[:m]
    Pw = pops.point_cloud(G, patches[:, :m], intrinsics, i)[:, :, c, c]                  # [1,m,4]
    points = (Pw[..., :3] / Pw[..., 3:]).reshape(m, 3)
    j = (i[:, None] + torch.arange(S, device=i.device)[None] - mid).clamp(0, N - 1).reshape(-1)
    live = local_weights.reshape(NM, S)[:m].sum(1) > 0
    tracked = patches_local[:, :m].reshape(1, m * S, 3, 1, 1)
    Wd = pops.point_cloud(G, tracked, intrinsics, j).reshape(m, S, 4)
    world = torch.zeros_like(patches_local)
    world[0, :m] = torch.where(live[:, None, None], points[:, None], Wd[..., :3] / Wd[..., 3:])
    Xc = G[:, j, None, None] * Pw[0][:, None].expand(m, S, 4).reshape(1, m * S, 1, 1, 4)
    trg = pops.proj(Xc, intrinsics[:, j], depth=True).reshape(m, S, 3)
    out = patches_local.clone()
    out[0, :m] = torch.where(live[:, None, None], trg, patches_local[0, :m])
    return points, world, out


# ---------------------------------------------------------------------------------- shared by the GPU tests and the bench tool
def to_gpu(d, dev="cuda:0"):
    """The arrays of a case / of random_inputs as the tensors pops.world_tracks takes (batch dimension 1)."""
    import torch
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    return dict(poses=t(d["poses"].astype(np.float32))[None], patches=t(d["patches"].astype(np.float32))[None],
                intrinsics=t(d["intrinsics"].astype(np.float32))[None], ix=t(d["ix"]),
                patches_local=t(d["patches_local"].astype(np.float32))[None], local_weights=t(d["local_weights"].astype(np.float32)),
                m=int(d["m"]))


def run_fused(g):
    """pops.world_tracks on a copy of the window buffer: (points [m,3], world [1,NM,S,3], patches_local_out [1,NM,S,3])."""
    from batrack_amd.backend import projective_ops as pops
    pl = g["patches_local"].clone()
    points, world = pops.world_tracks(g["poses"], g["patches"], g["intrinsics"], g["ix"], pl, g["local_weights"], g["m"])
    return points, world, pl


def fixture_case(D, c):
    return {k: D[f"{c}.{k}"] for k in ("poses", "intrinsics", "patches", "ix", "patches_local", "local_weights", "m")}


def parity_figures(got, ref, m, live, near=None):
    """The figures the gates are set on, of (points, world, patches_local_out) as float64 numpy against a reference:
    points / world / disp by rel_err (disp: live tracks, `near` left out), uv by uv_err (the same entries), and whether
    the finiteness of every output agrees exactly (`finite`) and the rows of patches_local that are not live or past m
    are equal (`rest`)."""
    keep = np.broadcast_to(live[:, None], got[2][:m].shape[:2]).copy()
    if near is not None:
        keep &= ~near
    uv, share = uv_err(got[2][:m][..., :2][keep], ref[2][:m][..., :2][keep])
    return dict(points=rel_err(got[0], ref[0]), world=rel_err(got[1], ref[1]),
                disp=rel_err(got[2][:m][..., 2][keep], ref[2][:m][..., 2][keep]), uv=uv, uv_share=share,
                finite=all(np.array_equal(np.isfinite(a), np.isfinite(b)) for a, b in zip(got, ref)),
                rest=np.array_equal(got[2][~np.pad(live, (0, len(got[2]) - m))], ref[2][~np.pad(live, (0, len(ref[2]) - m))]))


def caller_feedback(dev="cuda:0", n_frames=24, M=32, seed=3):
    """The replayed caller three times on one synthetic sequence — the fused step, the step composed from the older
    operations (a subclass), and the default without it: largest pose difference fused / composed, and the largest
    relative deviation of the live tracks' depth prior patches_local_[:, :, mid, 2] from their disparity patches_[:, :, 2]."""
    import torch
    import batrack_amd.backend.ba as hip_ba
    from batrack_amd.backend.lietorch import SE3
    from batrack_amd.sequence import SlamConfig, SyntheticObservations, WindowedBA

    class Composed(WindowedBA):
        def update_point_cloud(self):
            NM = self.N * self.M
            pl = self.patches_local_.view(1, NM, self.S_local, 3)
            points, world, out = composed_world_tracks(self.SE3, self.poses, self.patches, self.intrinsics, self.ix, pl,
                                                       self.patches_local_weights_, self.m)
            self.points_[:self.m] = points
            self.trajs_3d_world_.view(1, NM, self.S_local, 3)[:, :self.m] = world[:, :self.m]
            pl[:] = out

    def deviation(w):
        mid = (w.S_local + 1) // 2 - 1
        live = (w.patches_local_weights_.view(w.N * w.M, w.S_local)[:w.m].sum(1) > 0)
        prior = w.patches_local_.view(w.N * w.M, w.S_local, 3)[:w.m, mid, 2][live].double()
        d = w.patches_.view(w.N * w.M, 3)[:w.m, 2][live].double()
        return float(((prior - d).abs() / d.abs()).max()), int(live.sum())

    runs = {}
    for name, cls, on in (("fused", WindowedBA, True), ("composed", Composed, True), ("default", WindowedBA, False)):
        obs = SyntheticObservations(n_frames=n_frames, M=M, seed=seed)
        w = cls(obs, hip_ba.BA_rgbd_droid, SlamConfig(PATCHES_PER_FRAME=M, BUFFER_SIZE=n_frames + 1, UPDATE_POINT_CLOUD=on), device=dev)
        runs[name] = (w, w.run())
    w = runs["fused"][0]
    res = w.get_results()
    dev_f, live = deviation(w)
    written = int((w.trajs_3d_world_.view(w.N * w.M, -1) != 0).any(1).sum())
    return dict(pose_diff=float(np.abs(runs["fused"][1] - runs["composed"][1]).max()), dev_fused=dev_f,
                dev_composed=deviation(runs["composed"][0])[0], dev_default=deviation(runs["default"][0])[0], live=live, m=w.m,
                keys=len(res), trajs_2d_disp_is_buffer=bool(np.array_equal(res["trajs_2d_disp"], w.patches_local_[:w.counter].cpu().numpy())),
                points_finite=bool(torch.isfinite(w.points_[:w.m]).all()), world_rows_written=written)
