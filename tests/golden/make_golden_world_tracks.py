#!/usr/bin/env python3
"""Golden vectors for the end of the reference's per-frame update(): the world-frame point cloud, the tracks' 3-D
trajectories and the overwrite of the live tracks' window buffer (main/batrack.py:891-895, update_point_cloud :821-854).
Runs the reference's UNMODIFIED `BATRACK.update_point_cloud` on an `object.__new__(BATRACK)` whose buffers this script
fills (no __init__: it loads network weights), where the reference checkout is at hand.  The three statements
batrack.py:891-893 are not a method: they are stated here in this script's own words as what they are — the reference's
`pops.point_cloud` (called in place) over the first m tracks, and the centre pixel's first three components divided by
its fourth.

Stand-ins: tests/golden/refstubs (`cv2`, `lietorch_backends`, `cuda_corr`, `torch_scatter`) first on sys.path, and two empty
modules put into sys.modules here — `main.slam_visualizer` (LEAPVisualizer) and `main.frontend.md_tracker` (MDTracker) —
which batrack.py imports and this path never calls.  As for every BA fixture, the SE3 arithmetic below the reference's
Python wrapper is the stand-in's (our restatement of the published formulas): parity unpinned for it.  Everything above —
the gathers, the clamp of the frame index, the live mask, iproj / proj, which rows are overwritten — is the reference's.

Writes tests/golden/world_tracks.npz; per case c in (a, b, c), inputs rounded to float32 first:
  c.poses [N,7]  c.intrinsics [N,4]  c.patches [N*M,3,1,1]  c.ix [N*M]  c.patches_local [N*M,S_local,3]
  c.local_weights [N*M,S_local]  c.m  c.n  c.M  c.S_slam                                                   (inputs)
  c.points [m,3]  c.world [N*M,S_local,3]  c.patches_local_out [N*M,S_local,3]        (float64 run of the reference)
  c.points32, c.world32, c.patches_local_out32                                         (its float32 run)
  c.near_clamp [m,S_local] bool   live entries whose camera-frame depth is within 1e-5 of the 1e-2 clamp in the float64 run
  gate.c.points, gate.c.world, gate.c.disp   e32 = max |ref32 - ref64| / (1 + |ref64|) over the finite entries (disp: the
                                             third column of patches_local_out, live tracks, near_clamp left out)
Cases: (a) a mid-sequence buffer, n < N, live and not-live tracks, never-filled slots, source frames at both ends of the
buffer; (b) points behind window cameras (the clamp); (c) intrinsics that differ between frames.
Only inputs we generated and numeric outputs are written.

    python tests/golden/make_golden_world_tracks.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path[:0] = [os.path.join(HERE, "refstubs"), os.path.join(REF, "main"), REF, ROOT]
for name, attr in (("main.slam_visualizer", "LEAPVisualizer"), ("main.frontend.md_tracker", "MDTracker")):
    mod = types.ModuleType(name)
    setattr(mod, attr, type(attr, (), {}))
    sys.modules[name] = mod

import main.batrack as ref_batrack                     # noqa: E402  (reference, unmodified)
from main.backend import projective_ops as ref_pops    # noqa: E402
from main.backend.lietorch import SE3 as RefSE3        # noqa: E402

from batrack_amd import graphgen                       # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import world_util                                      # noqa: E402  (only for near_clamp: the camera-frame depth)

torch.set_num_threads(4)


def f32r(a):
    return np.asarray(a, np.float32).astype(np.float64)


def make_inputs(seed, N, M, S_slam, n, step, d_range, vary_K):
    """A camera moving `step` per frame through tracked points; about 70 % of the tracks live."""
    rng = np.random.default_rng(seed)
    S = 2 * S_slam - 1
    mid = (S + 1) // 2 - 1
    NM, m = N * M, n * M
    s = np.arange(N)[:, None]
    xi = s * step * np.array([0.5, 0.1, 1.0, 0.0, 0.1, 0.02]) + np.sin(s * 0.7) * np.array([0.0, 0.04, 0.0, 0.01, 0.0, 0.02])
    poses = graphgen.se3_exp(xi)
    poses[:, 3:] *= rng.uniform(0.7, 1.4, (N, 1))                    # not unit: re-normalised on load
    K = np.tile(np.array([320.0, 310.0, 160.0, 120.0]), (N, 1))
    if vary_K:
        K = K * rng.uniform(0.8, 1.25, (N, 4))
    patches = np.stack([rng.uniform(10, 310, NM), rng.uniform(10, 230, NM), rng.uniform(*d_range, NM)], 1)
    ix = np.arange(NM) // M
    far = rng.choice(m, 12, replace=False)                           # tracks whose source frame is at the end of the buffer
    ix[far[:6]], ix[far[6:]] = N - 1, N - 2
    poses, K, patches = f32r(poses), f32r(K), f32r(patches)
    # the tracker's (u, v, disparity) in the window frames: the track's reprojection + noise
    jj = np.clip(ix[:, None] + np.arange(S)[None] - mid, 0, N - 1)
    kk = np.repeat(np.arange(NM), S)
    u, v, Z = graphgen.reproject(poses, patches, K, np.repeat(ix, S), jj.reshape(-1), kk)
    pl = np.stack([u + rng.normal(0, 1.0, u.shape), v + rng.normal(0, 1.0, u.shape),
                   patches[kk, 2] / np.maximum(Z, 0.05) * (1.0 + rng.normal(0, 0.05, u.shape))], 1).reshape(NM, S, 3)
    live = rng.random(NM) < 0.7
    w = rng.uniform(0.1, 1.0, (NM, S)) * (rng.random((NM, S)) < 0.6)
    w[live, mid] = 0.5                                               # a live track has at least one slot > 0
    w[~live] = 0.0
    never = (rng.random((NM, S)) < 0.25) & ~live[:, None]            # slots the tracker never filled
    pl[never] = 0.0
    return dict(poses=poses, intrinsics=K, patches=patches.reshape(NM, 3, 1, 1), ix=ix.astype(np.int64),
                patches_local=f32r(pl), local_weights=f32r(w), m=m, n=n, M=M, S_slam=S_slam, N=N)


def run_reference(d, dtype):
    """update() :891-895 on buffers we fill: (points [m,3], trajs_3d_world [NM,S,3], patches_local [NM,S,3])."""
    N, M, S_slam, n = d["N"], d["M"], d["S_slam"], d["n"]
    o = object.__new__(ref_batrack.BATRACK)
    o.P, o.N, o.M, o.n, o.m, o.S_local = 1, N, M, n, d["m"], 2 * S_slam - 1
    t = lambda a: torch.as_tensor(np.array(a), dtype=dtype)
    o.poses_ = t(d["poses"])
    o.intrinsics_ = t(d["intrinsics"])
    o.patches_ = t(d["patches"]).reshape(N, M, 3, 1, 1)
    o.index_ = torch.as_tensor(d["ix"]).reshape(N, M)
    o.patches_local_ = t(d["patches_local"]).reshape(N, M, o.S_local, 3)
    o.patches_local_weights_ = t(d["local_weights"]).reshape(N, M, o.S_local, 1)
    o.trajs_3d_world_ = torch.zeros(N, M, o.S_local, 3, dtype=dtype)
    o.points_ = torch.zeros(N * M, 3, dtype=dtype)
    with torch.no_grad():
        # batrack.py:891-893 in our words: the world points of the first m tracks, centre pixel, de-homogenised
        hom = ref_pops.point_cloud(RefSE3(o.poses), o.patches[:, :o.m], o.intrinsics, o.ix[:o.m])
        c = o.P // 2
        pts = (hom[..., c, c, :3] / hom[..., c, c, 3:]).reshape(-1, 3)
        o.points_[:len(pts)] = pts
        o.update_point_cloud()                                        # :895, the reference's method as it lies there
    g = lambda x: x.reshape(N * M, *x.shape[2:]).numpy().astype(np.float64)
    return o.points_[:o.m].numpy().astype(np.float64), g(o.trajs_3d_world_), g(o.patches_local_)


def main():
    out = {}
    specs = dict(a=dict(seed=21, N=12, M=16, S_slam=4, n=9, step=0.05, d_range=(0.2, 1.0), vary_K=False),
                 b=dict(seed=22, N=12, M=16, S_slam=4, n=9, step=0.35, d_range=(0.5, 6.0), vary_K=False),
                 c=dict(seed=23, N=10, M=24, S_slam=3, n=8, step=0.05, d_range=(0.2, 1.0), vary_K=True))
    for c, spec in specs.items():
        d = make_inputs(**spec)
        p64, w64, l64 = run_reference(d, torch.float64)
        p32, w32, l32 = run_reference(d, torch.float32)
        m = d["m"]
        live = d["local_weights"][:m].sum(1) > 0
        Xc3 = world_util.np_world_tracks(d["poses"], d["intrinsics"], d["patches"], d["ix"], d["patches_local"],
                                         d["local_weights"], m)[3]
        near = live[:, None] & (np.abs(Xc3 - world_util.CLAMP) < 1e-5)
        for k in ("poses", "intrinsics", "patches", "patches_local", "local_weights"):
            out[f"{c}.{k}"] = d[k].astype(np.float32)
        out[f"{c}.ix"] = d["ix"]
        for k in ("m", "n", "M", "S_slam"):
            out[f"{c}.{k}"] = np.int64(d[k])
        out[f"{c}.points"], out[f"{c}.world"], out[f"{c}.patches_local_out"] = p64, w64, l64
        out[f"{c}.points32"], out[f"{c}.world32"], out[f"{c}.patches_local_out32"] = (x.astype(np.float32) for x in (p32, w32, l32))
        out[f"{c}.near_clamp"] = near
        keep = live[:, None] & ~near
        out[f"gate.{c}.points"] = np.float64(world_util.rel_err(p32, p64))
        out[f"gate.{c}.world"] = np.float64(world_util.rel_err(w32, w64))
        out[f"gate.{c}.disp"] = np.float64(world_util.rel_err(l32[:m, :, 2][keep], l64[:m, :, 2][keep]))
        same_fin = np.array_equal(np.isfinite(w32), np.isfinite(w64))
        behind = live[:, None] & (Xc3 < world_util.CLAMP)
        uv = world_util.uv_err(l32[:m, :, :2][keep], l64[:m, :, :2][keep])
        print(f"case {c}: m {m} of {d['N'] * d['M']}, live {int(live.sum())}, non-finite world rows {int((~np.isfinite(w64)).any(-1).sum())}, "
              f"same finiteness in float32 {same_fin}, clamped entries {int(behind.sum())}, near clamp {int(near.sum())} "
              f"({near.sum() / max(live.sum() * Xc3.shape[1], 1):.2%}), e32 points {out[f'gate.{c}.points']:.2e} world "
              f"{out[f'gate.{c}.world']:.2e} disp {out[f'gate.{c}.disp']:.2e}, (u, v) float32 run on the project's gate {uv[0]:.2e}")
    path = os.path.join(HERE, "world_tracks.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
