#!/usr/bin/env python3
"""Golden vectors for the last step of a frame: the reference's `BATRACK.keyframe` (main/batrack.py:1026-1073) and,
through it, `motionmag` (:1011-1018), `remove_factors` (:206-212) and `pops.flow_mag` (backend/projective_ops.py:112-122),
all UNMODIFIED, on an `object.__new__(BATRACK)` whose buffers this script fills (no __init__: it loads network weights),
where the reference checkout is at hand (BATRACK_REFERENCE, default /root/reference).  float32, CPU.

Stand-ins: tests/golden/refstubs first on sys.path and the two empty modules `main.slam_visualizer` and
`main.frontend.md_tracker`, as for the observe fixture; the SE3 arithmetic below the reference's Python wrapper is the
stand-in's.  `motionmag` is wrapped ON THE INSTANCE only to record what it returns — with one exception, cases (c) and
(d): for a pair WITHOUT edges the reference's method raises inside its lietorch wrapper (groups.py:130 cannot `view` a group
tensor of no elements), so no run of it exists; the wrapper answers such a pair with NaN, what `flow.mean()` gives for an
empty `flow`, and the reference's comparison `m / 2 < KEYFRAME_THRESH` then keeps the frame.  Every pair that has edges
goes through the reference's method.

Writes tests/golden/keyframe.npz.  Per case c, with X one of the six edge arrays (ii, jj, kk, targets_3d, weights,
weights_pose) or of the eleven buffers (tstamps, colors, poses, patches, intrinsics, patches_local, patches_local_vis,
patches_local_static, patches_local_weights, patches_valid, trajs_3d_world):
  c.X_in, c.X_out      the state before and after;   c.n_in, c.m_in, c.n_out, c.m_out
  c.M, c.kf_stride, c.KEYFRAME_INDEX, c.KEYFRAME_THRESH, c.REMOVAL_WINDOW
  c.mags [2]           what the two motionmag calls returned (NaN, NaN when keyframe() returned before them)
  c.removed            whether the frame left the buffer
  c.delta_t [r,2], c.delta_dP [r,7]     `delta` afterwards: (t1, t0) and dP of every entry (r = 0 or 1)
Cases: (a) removed: kf_stride 1, KEYFRAME_INDEX 4, edges on both sides of k and at k as source and as target, duplicates,
sources at exactly n - REMOVAL_WINDOW - 1 and n - REMOVAL_WINDOW (the window uses the new n); (b) kept: the same state, a
lower threshold, only the removal window applies; (c) empty pair: no edge (k+1 -> k), the mean is NaN, kept; (d) k = 0;
(e) early return: k % kf_stride != 0, everything untouched, old sources included; (f) kf_stride 2, KEYFRAME_INDEX 3,
removed.  In every case that decides, |m/2 - thresh| >= 0.5 px (asserted): no summation order can flip it.
Only generated inputs and numeric outputs are written.

    python tests/golden/make_golden_keyframe.py
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

from batrack_amd import graphgen                       # noqa: E402

import keyframe_util as ku                             # noqa: E402  (only the names)

torch.set_num_threads(4)
N, M, S_LOCAL, RW = 16, 8, 11, 8


class Settings:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __contains__(self, k):
        return k in self.__dict__


def make_state(seed, n):
    """A camera moving through tracked points; edges (track of frame f -> frames within 3 of f) of every source frame from 1
    on, a tenth of them twice, in random order; buffers whose rows are all different."""
    rng = np.random.default_rng(seed)
    s = np.arange(N)[:, None]
    xi = s * 0.06 * np.array([0.5, 0.1, 1.0, 0.0, 0.1, 0.02]) + np.sin(s * 0.7) * np.array([0.0, 0.04, 0.0, 0.01, 0.0, 0.02])
    poses = graphgen.se3_exp(xi).astype(np.float32)
    K = (np.tile(np.array([320.0, 310.0, 160.0, 120.0]), (N, 1)) * rng.uniform(0.95, 1.05, (N, 4))).astype(np.float32)
    patches = np.stack([rng.uniform(10, 310, (N, M)), rng.uniform(10, 230, (N, M)), rng.uniform(0.2, 1.0, (N, M))], 2).astype(np.float32)
    ii, jj, kk = [], [], []
    for f in range(1, n):
        for t in range(M):
            if rng.random() < 0.25:
                continue
            for j in range(max(f - 3, 0), min(f + 3, n - 1) + 1):
                ii.append(f); jj.append(j); kk.append(f * M + t)
    ii, jj, kk = (np.array(a, np.int64) for a in (ii, jj, kk))
    dup = rng.choice(ii.size, ii.size // 10, replace=False)
    ii, jj, kk = (np.concatenate([a, a[dup]]) for a in (ii, jj, kk))
    perm = rng.permutation(ii.size)
    ii, jj, kk = ii[perm], jj[perm], kk[perm]
    E = ii.size
    rows = lambda shape, base: (base + np.arange(N).reshape(N, *[1] * (len(shape) - 1)) + rng.integers(0, 4, shape) * 0.25).astype(np.float32)
    bufs = dict(tstamps=(np.arange(N) * 3 + 1).astype(np.int64), colors=rng.integers(0, 255, (N, M, 3)).astype(np.uint8),
                poses=poses, patches=patches.reshape(N, M, 3, 1, 1), intrinsics=K,
                patches_local=rows((N, M, S_LOCAL, 3), 100.0), patches_local_vis=rows((N, M, S_LOCAL, 1), 200.0),
                patches_local_static=rows((N, M, S_LOCAL, 1), 300.0), patches_local_weights=rows((N, M, S_LOCAL, 1), 400.0),
                patches_valid=rows((N, M), 500.0), trajs_3d_world=rows((N, M, S_LOCAL, 3), 600.0))
    edges = dict(ii=ii, jj=jj, kk=kk, targets_3d=(np.arange(E)[:, None] + np.array([0.0, 0.25, 0.5])).astype(np.float32),
                 weights=(rng.random((E, 2)) < 0.8).astype(np.float32), weights_pose=(rng.random((E, 2)) < 0.5).astype(np.float32))
    return bufs, edges


def run_case(bufs, edges, n, kf_stride, index, thresh):
    o = object.__new__(ref_batrack.BATRACK)
    o.cfg = Settings(slam=Settings(KEYFRAME_INDEX=index, KEYFRAME_THRESH=thresh, REMOVAL_WINDOW=RW))
    o.P, o.N, o.M, o.n, o.m, o.kf_stride, o.S_local = 1, N, M, n, n * M, kf_stride, S_LOCAL
    t = lambda a: torch.as_tensor(np.array(a))
    for name in ku.BUFFERS:
        setattr(o, name + "_", t(bufs[name]))
    o.index_ = (torch.arange(N * M) // M).reshape(N, M)
    o.ii, o.jj, o.kk = t(edges["ii"]), t(edges["jj"]), t(edges["kk"])
    o.targets_3d, o.weights, o.weights_pose = (t(edges[k])[None] for k in ("targets_3d", "weights", "weights_pose"))
    o.delta = {}
    o.local_window, o.local_window_depth = list(range(8)), list(range(8))
    mags = []
    inner = o.motionmag                                     # the reference's bound method

    def recording(i, j):
        if not bool(((o.ii == i) & (o.jj == j)).any()):
            mags.append(float("nan"))                       # see the module's text: torch.mean of nothing, without the view that raises
        else:
            mags.append(inner(i, j))
        return mags[-1]
    o.motionmag = recording
    with torch.no_grad():
        o.keyframe()                                        # the reference's method as it lies there
    out = {name + "_out": getattr(o, name + "_").numpy().copy() for name in ku.BUFFERS}
    out.update(ii_out=o.ii.numpy().copy(), jj_out=o.jj.numpy().copy(), kk_out=o.kk.numpy().copy(),
               targets_3d_out=o.targets_3d[0].numpy().copy(), weights_out=o.weights[0].numpy().copy(),
               weights_pose_out=o.weights_pose[0].numpy().copy(), n_out=np.int64(o.n), m_out=np.int64(o.m),
               mags=np.array(mags + [np.nan] * (2 - len(mags)), np.float64), removed=np.bool_(o.n != n),
               delta_t=np.array([[t1, t0] for t1, (t0, _) in o.delta.items()], np.int64).reshape(-1, 2),
               delta_dP=np.array([dP.data.numpy().reshape(7) for _, dP in o.delta.values()], np.float32).reshape(-1, 7))
    for k, v in list(bufs.items()) + list(edges.items()):
        out[k + "_in"] = v
    out.update(n_in=np.int64(n), m_in=np.int64(n * M), M=np.int64(M), kf_stride=np.int64(kf_stride), KEYFRAME_INDEX=np.int64(index),
               KEYFRAME_THRESH=np.float64(thresh), REMOVAL_WINDOW=np.int64(RW))
    return out, len(mags)


def main():
    n = 14
    bufs, edges = make_state(41, n)
    k = n - 4
    src = edges["ii"]
    assert (src == n - RW - 1).any() and (src == n - RW).any() and (src == k).any() and (edges["jj"] == k).any()
    assert ((src > k) & (edges["jj"] < k)).any() and ((src < k) & (edges["jj"] > k)).any()
    probe, _ = run_case(bufs, edges, n, 1, 4, 1e9)
    half = probe["mags"].sum() / 2
    no_next = {name: v[~((edges["ii"] == k + 1) & (edges["jj"] == k))] for name, v in edges.items()}
    bufs4, edges4 = make_state(42, 4)
    probe_f, _ = run_case(bufs, edges, 13, 2, 3, 1e9)
    half_f = probe_f["mags"].sum() / 2
    specs = dict(a=(bufs, edges, n, 1, 4, half + 1.0), b=(bufs, edges, n, 1, 4, half - 1.0), c=(bufs, no_next, n, 1, 4, 1e6),
                 d=(bufs4, edges4, 4, 1, 4, 1e6), e=(bufs, edges, n, 2, 3, 1e6), f=(bufs, edges, 13, 2, 3, half_f + 1.0))
    assert tuple(specs) == ku.CASES
    want = dict(a=True, b=False, c=False, d=False, e=False, f=True)
    out = {}
    for c, spec in specs.items():
        r, calls = run_case(*spec)
        m2 = r["mags"].sum() / 2
        assert bool(r["removed"]) == want[c], c
        assert calls == (0 if c == "e" else 2)
        if np.isfinite(m2):
            assert abs(m2 - spec[5]) >= 0.5, (c, m2, spec[5])     # the margin no summation order can cross
        print(f"case {c}: n {int(r['n_in'])} -> {int(r['n_out'])}, E {r['ii_in'].size} -> {r['ii_out'].size}, mags {r['mags']}, "
              f"m/2 {m2:.4f} against {spec[5]:.4f}, removed {bool(r['removed'])}, delta {r['delta_t'].tolist()}")
        for name, v in r.items():
            out[f"{c}.{name}"] = v
    path = os.path.join(HERE, "keyframe.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "observe_window.npz"))


if __name__ == "__main__":
    main()
