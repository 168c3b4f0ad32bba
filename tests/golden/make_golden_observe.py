#!/usr/bin/env python3
"""Golden vectors for the step between the tracker's forward pass and the bundle adjustment: the reference's
`predict_target` (main/batrack.py:760-818) and, through it, `get_window_trajs` (:667-757), `get_queries` (:459-480),
`_compute_sparse_tracks` (:529-587), `bilinear_sample2d` (frontend/core/model_utils.py:75-158) and `update_local`
(:632-663), all UNMODIFIED, on an `object.__new__(BATRACK)` whose buffers this script fills (no __init__: it loads
network weights), where the reference checkout is at hand (BATRACK_REFERENCE, default /root/reference).  float32, CPU.

Stand-ins: tests/golden/refstubs first on sys.path, the two empty modules `main.slam_visualizer` and
`main.frontend.md_tracker` (as for the world-tracks fixture); `self.network`, a function that returns clones of the
tensors prepared here in the tuple layout of md_tracker (tracks, _, depths, static tracks, visibilities, dynamic, _);
`self.visualizer`, whose add_track does nothing; `self.cfg`, a minimal settings object with attribute access and `in`.

Writes tests/golden/observe_window.npz.  `dmaps` [6, H, W] is shared: a case uses its first S' maps.  Per case c:
  c.traj [S,Nq,2]  c.depth, c.vis, c.dyn [S,Nq]      what the network returns (512 x 384 coordinates)
  c.queries [Nq,3]                                    get_queries(): (t, x, y)
  c.ii, c.jj, c.kk [E]   c.patches_valid_in [N,M]   c.<buffer>_in   (the five window buffers, [N*M,S_local(,3)])
  c.n, c.Sp, c.M, c.kf_stride, c.wd, c.ht, c.is_initialized, c.VIS_THRESHOLD, c.STATIC_THRESHOLD, c.STATIC_QUANTILE, c.MIN_TRACK_LEN
  c.targets_3d [E,3]  c.weights, c.weights_pose [E,2]  c.query_disp [Nq]  c.patches_valid_out  c.<buffer>_out
Cases: (a) an initialised full window; (b) start-up, S' < S, n < MIN_TRACK_LEN, not initialised; (c_below, c_above)
STATIC_QUANTILE 0.3 with the quantile below / above STATIC_THRESHOLD, a window buffer shorter than 2S-1 so that slots fall
outside it; (d_len, d_init) ties and edges — coordinates exactly at pad and wd-pad, vis exactly at the threshold, static
scores exactly equal to the threshold, exactly MIN_TRACK_LEN and one fewer visible frames (d_len), exactly 3 and 4
labelled frames under the initialised rule alone (d_init: MIN_TRACK_LEN > n), NaN depth, a NaN coordinate, a depth below
1e-2, queries outside the depth map; (e) case (a) with a NaN in the dynamic scores.
Only generated inputs and numeric outputs are written.

    python tests/golden/make_golden_observe.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("BATRACK_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(HERE, "refstubs"), os.path.join(REF, "main"), REF, ROOT, os.path.join(ROOT, "tests")]
for name, attr in (("main.slam_visualizer", "LEAPVisualizer"), ("main.frontend.md_tracker", "MDTracker")):
    mod = types.ModuleType(name)
    setattr(mod, attr, type(attr, (), {}))
    sys.modules[name] = mod

import main.batrack as ref_batrack                     # noqa: E402  (reference, unmodified)

import observe_util as ou                              # noqa: E402  (only window_edges and the names)

torch.set_num_threads(4)
H, W, IH, IW, PAD = 52, 64, 384, 512, 20               # W / 512 is a power of two (exact ties in x), H / 384 is not
N, M, S, KF = 16, 8, 6, 2


class Settings:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __contains__(self, k):
        return k in self.__dict__


def preimage(target, r):
    """A float32 v with f32(v * r) == target exactly."""
    r, target = np.float32(r), np.float32(target)
    v = np.float32(target / r)
    for _ in range(64):
        p = np.float32(v * r)
        if p == target:
            return v
        v = np.nextafter(v, np.float32(np.inf if p < target else -np.inf), dtype=np.float32)
    raise RuntimeError("no preimage")


def make_case(seed, Sp, n, init, cfg, S_local=2 * S - 1, dyn_kind="mixed", edges=False, nan_dyn=False):
    rng = np.random.default_rng(seed)
    Q = -(-Sp // KF)
    Nq = Q * M
    rx, ry = np.float32(W / IW), np.float32(H / IH)
    # the tracker's output in its 512 x 384 frame: tracks that wander in and out of the padded image
    base = np.stack([rng.uniform(16, W - 16, Nq) / rx, rng.uniform(18, H - 18, Nq) / ry], 1)
    traj = base[None] + np.cumsum(rng.normal(0, 1.0, (S, Nq, 2)) * np.array([8.0, 6.0]), 0)
    depth = rng.uniform(0.3, 6.0, (S, Nq))
    vis = np.where(rng.random((S, Nq)) < 0.7, rng.uniform(0.9, 1.0, (S, Nq)), rng.uniform(0.0, 0.9, (S, Nq)))
    if dyn_kind == "mixed":                                 # most tracks static, some clearly moving
        dyn = np.where(rng.random((1, Nq)) < 0.7, rng.uniform(0.0, 0.3, (S, Nq)), rng.uniform(0.85, 1.0, (S, Nq)))
    elif dyn_kind == "moving":                              # static scores below STATIC_THRESHOLD almost everywhere
        dyn = rng.uniform(0.93, 1.0, (S, Nq))
    else:                                                   # "still"
        dyn = rng.uniform(0.0, 0.5, (S, Nq))
    traj, depth, vis, dyn = (np.asarray(a, np.float32) for a in (traj, depth, vis, dyn))
    patches_xy = np.stack([rng.uniform(2, W - 2, (N, M)), rng.uniform(2, H - 2, (N, M))], -1).astype(np.float32)
    lo = n - Sp
    if edges:
        fr = lambda q: [s for s in range(Sp) if s != KF * (q // M)]          # the frames the tail does not overwrite
        vt = np.float32(cfg.slam.VIS_THRESHOLD)
        hi_v, lo_v = np.float32(0.99), np.float32(0.2)
        inside = np.array([preimage(30.0, rx), preimage(30.0, ry)], np.float32)
        # tracks 0-3: coordinates exactly at the bounds, on visible frames
        for q, (col, val, r) in enumerate(((0, PAD, rx), (0, W - PAD, rx), (1, PAD, ry), (1, H - PAD, ry))):
            for s in fr(q):
                traj[s, q] = inside
                vis[s, q] = hi_v
            traj[fr(q)[0], q, col] = preimage(val, r)
            traj[fr(q)[1], q, col] = np.nextafter(preimage(val, r), np.float32(-np.inf), dtype=np.float32)
        # track 4: vis exactly at the threshold (strict: not visible), its neighbour just above
        for s in fr(4):
            traj[s, 4] = inside
        vis[fr(4), 4] = [vt, np.nextafter(vt, np.float32(2), dtype=np.float32), vt, hi_v, vt][:len(fr(4))]
        # tracks 5, 6: exactly MIN_TRACK_LEN and one fewer visible-and-inside frames (the query frame counts when inside)
        # tracks 8, 9: exactly 4 and 3 labelled frames (the query frame is labelled always)
        for q, k in ((5, cfg_len(cfg)), (6, cfg_len(cfg) - 1), (8, 4), (9, 3)):
            own = KF * (q // M)
            patches_xy[lo + own, q % M] = (31.5, 22.25)                          # the query itself inside
            for i, s in enumerate(fr(q)):
                traj[s, q] = inside
                vis[s, q] = hi_v if i < k - 1 else lo_v
        # track 10: NaN depth and a depth below 1e-2; track 11: a NaN coordinate
        for s in fr(10):
            traj[s, 10] = traj[s, 11] = inside
        vis[:, 10] = vis[:, 11] = hi_v
        depth[fr(10)[0], 10], depth[fr(10)[1], 10], depth[fr(10)[2], 10] = np.nan, 1e-3, -2.0
        traj[fr(11)[0], 11, 0] = np.nan
        traj[fr(11)[1], 11, 1] = np.nan
        # queries of the third keyframe outside the depth map and on its last row / column
        patches_xy[lo + 2 * KF, 4] = (-3.5, 10.25)
        patches_xy[lo + 2 * KF, 5] = (W + 1.75, H + 0.5)
        patches_xy[lo + 2 * KF, 6] = (W - 1.0, H - 1.0)
        patches_xy[lo + 2 * KF, 7] = (W - 0.5, -0.25)
        # two static scores equal to the largest one: with STATIC_QUANTILE 0 and all scores below STATIC_THRESHOLD the
        # threshold is that value
        top = dyn.min()
        dyn[2, 1] = dyn[4, 7] = top
    if nan_dyn:
        dyn[S - 1, 3] = np.nan                              # on a padded / last frame: it still poisons the quantile
    dmaps = DMAPS[:Sp]
    o = object.__new__(ref_batrack.BATRACK)
    o.cfg = cfg
    o.P, o.N, o.M, o.n, o.S, o.S_slam, o.kf_stride, o.S_local = 1, N, M, n, S, S, KF, S_local
    o.interp_shape, o.wd, o.ht, o.is_initialized = (IH, IW), W, H, init
    t = lambda a: torch.as_tensor(np.array(a))
    o.patches_ = torch.zeros(N, M, 3, 1, 1)
    o.patches_[:, :, :2, 0, 0] = t(patches_xy)
    o.patches_[:, :, 2] = 1.0
    o.local_window = [torch.zeros(3, H, W) for _ in range(Sp)]
    o.local_window_depth = [t(dmaps[s])[None] for s in range(Sp)]
    pv_in = (rng.random((N, M)) < 0.3).astype(np.float32)
    pv_in[0, 0] = 0.5                                       # any non-zero value counts as valid
    if edges:
        pv_in[lo + KF, 0] = pv_in[lo + KF, 1] = 0.0         # tracks 8, 9: only the rule decides
    o.patches_valid_ = t(pv_in)
    o.patches_monodisp_ = torch.zeros(N, M, 1)
    # what the buffers hold before: a few distinct values (the file stays small), none of which the step can write
    few = lambda base, shape: base + rng.integers(0, 8, shape) * 0.125
    bufs_in = dict(patches_local=few(-9.0, (N * M, S_local, 3)), local_monodisp=few(-5.0, (N * M, S_local)),
                   local_vis=few(2.0, (N * M, S_local)), local_static=few(3.0, (N * M, S_local)), local_weights=few(4.0, (N * M, S_local)))
    bufs_in = {k: v.astype(np.float32) for k, v in bufs_in.items()}
    o.patches_local_ = t(bufs_in["patches_local"]).reshape(N, M, S_local, 3)
    o.patches_local_monodisp_ = t(bufs_in["local_monodisp"]).reshape(N, M, S_local, 1)
    o.patches_local_vis_ = t(bufs_in["local_vis"]).reshape(N, M, S_local, 1)
    o.patches_local_static_ = t(bufs_in["local_static"]).reshape(N, M, S_local, 1)
    o.patches_local_weights_ = t(bufs_in["local_weights"]).reshape(N, M, S_local, 1)
    o.targets_3d, o.weights, o.weights_pose = torch.zeros(1, 0, 3), torch.zeros(1, 0, 2), torch.zeros(1, 0, 2)
    o.ii_new, o.jj_new, o.kk_new = ou.window_edges(n, Sp, M, KF)
    o.visualizer = Settings(add_track=lambda data: None)
    seen = {}

    def network(rgbds, queries, iters):
        assert rgbds.shape[1] == S and queries.shape[1] == Nq
        seen["queries"] = queries.clone()
        return (t(traj)[None].clone(), None, t(depth)[None, ..., None].clone(), None, t(vis)[None].clone(), t(dyn)[None].clone(), None)
    o.network = network
    queries = o.get_queries()[0].numpy().copy()
    with torch.no_grad():
        o.predict_target()                                  # the reference's method as it lies there
    E = Nq * Sp
    assert o.targets_3d.shape == (1, E, 3) and o.weights.shape == (1, E, 2) and o.weights_pose.shape == (1, E, 2)
    flat = lambda x: x.reshape(N * M, *x.shape[2:]).numpy().copy()
    out = dict(traj=traj, depth=depth, vis=vis, dyn=dyn, queries=queries.astype(np.float32),
               ii=o.ii_new.numpy(), jj=o.jj_new.numpy(), kk=o.kk_new.numpy(), patches_valid_in=pv_in,
               n=np.int64(n), Sp=np.int64(Sp), M=np.int64(M), kf_stride=np.int64(KF), wd=np.int64(W), ht=np.int64(H),
               is_initialized=np.bool_(init), VIS_THRESHOLD=np.float64(cfg.slam.VIS_THRESHOLD if "VIS_THRESHOLD" in cfg.slam else np.nan),
               STATIC_THRESHOLD=np.float64(cfg.slam.STATIC_THRESHOLD), STATIC_QUANTILE=np.float64(cfg.slam.STATIC_QUANTILE),
               MIN_TRACK_LEN=np.int64(cfg.slam.MIN_TRACK_LEN),
               targets_3d=o.targets_3d[0].numpy(), weights=o.weights[0].numpy(), weights_pose=o.weights_pose[0].numpy(),
               query_disp=o.patches_monodisp_[lo:n:KF].reshape(-1).numpy().copy(), patches_valid_out=o.patches_valid_.numpy().copy(),
               patches_local_out=flat(o.patches_local_), local_monodisp_out=flat(o.patches_local_monodisp_)[..., 0],
               local_vis_out=flat(o.patches_local_vis_)[..., 0], local_static_out=flat(o.patches_local_static_)[..., 0],
               local_weights_out=flat(o.patches_local_weights_)[..., 0])
    for k, v in bufs_in.items():
        out[k + "_in"] = v
    th = ou.static_threshold(torch.as_tensor(dyn), cfg.slam.STATIC_QUANTILE, cfg.slam.STATIC_THRESHOLD)
    w0 = out["weights"][:, 0]
    print(f"  S' {Sp} n {n} Nq {Nq} E {E}: threshold {th!r}, weights > 0 {int((w0 > 0).sum())}, pose weights > 0 "
          f"{int((out['weights_pose'][:, 0] > 0).sum())}, valid rows changed {int((out['patches_valid_out'] != pv_in).sum())}, "
          f"NaN targets {int(np.isnan(out['targets_3d']).sum())}, slots written {int((out['local_vis_out'] < 2).sum())} of {E}")
    return out


def cfg_len(cfg):
    return cfg.slam.MIN_TRACK_LEN if cfg.slam.MIN_TRACK_LEN <= S else 3


def settings(**slam):
    base = dict(VIS_THRESHOLD=0.9, STATIC_THRESHOLD=0.1, STATIC_QUANTILE=0.0, MIN_TRACK_LEN=3, S_slam=S, backward_tracking=False)
    base.update(slam)
    return Settings(slam=Settings(**base), model=Settings(mode="md_tracker", I=4, S=S))


def main():
    global DMAPS
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    DMAPS = np.stack([2.5 + 1.5 * np.sin(0.21 * xx + 0.4 * s) * np.cos(0.17 * yy - 0.3 * s) + rng.integers(-8, 9, (H, W)) / 128.0
                      for s in range(S)]).astype(np.float32)
    DMAPS[0, :6, :6] = 0.004                                 # a corner below the 1e-2 clamp
    specs = dict(
        a=dict(seed=31, Sp=S, n=10, init=True, cfg=settings()),
        b=dict(seed=32, Sp=3, n=3, init=False, cfg=settings(MIN_TRACK_LEN=4)),
        c_below=dict(seed=33, Sp=S, n=12, init=True, cfg=settings(STATIC_QUANTILE=0.3), S_local=5, dyn_kind="moving"),
        c_above=dict(seed=34, Sp=S, n=12, init=True, cfg=settings(STATIC_QUANTILE=0.3), S_local=5, dyn_kind="still"),
        d_len=dict(seed=35, Sp=S, n=10, init=True, cfg=settings(), dyn_kind="moving", edges=True),
        d_init=dict(seed=35, Sp=S, n=10, init=True, cfg=settings(MIN_TRACK_LEN=11), dyn_kind="moving", edges=True),
        e=dict(seed=31, Sp=S, n=10, init=True, cfg=settings(), nan_dyn=True))
    assert tuple(specs) == ou.CASES
    out = {"dmaps": DMAPS}
    for c, spec in specs.items():
        print("case", c)
        for k, v in make_case(**spec).items():
            out[f"{c}.{k}"] = v
    path = os.path.join(HERE, "observe_window.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
