"""Degenerate BA problems shared by the CPU (plan emulator) and GPU edge-case tests; graphs of a particular shape shared by the
CPU planner tests and the GPU tests that step them."""
import numpy as np

import oracle
from batrack_amd import graphgen


def problem(ii, jj, kk, n_buf, p_tot, seed=0, target_shift=0.0):
    rng = np.random.default_rng(seed)
    K = np.tile(np.array([500.0, 500.0, 320.0, 240.0]), (n_buf, 1))
    poses = np.zeros((n_buf, 7)); poses[:, 6] = 1.0
    poses[:, 0] = 0.05 * np.arange(n_buf)
    q = 0.01 * rng.standard_normal((n_buf, 4)) + np.array([0, 0, 0, 1.0])
    poses[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    patches = np.stack([rng.uniform(100, 540, p_tot), rng.uniform(80, 400, p_tot), rng.uniform(0.2, 1.0, p_tot)], 1)
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    d = dict(poses=f(poses), patches=f(patches), mono=f(patches[:, 2] * 1.05), intrinsics=f(K), ii=np.asarray(ii, np.int64), jj=np.asarray(jj, np.int64),
             kk=np.asarray(kk, np.int64), bounds=np.array([0.0, 0.0, 640.0, 480.0]))
    E = len(d["ii"])
    # targets: the reprojection of the current state plus noise (so that the residuals are small and valid) [+ a shift]
    e = oracle.edges(d["poses"], d["patches"], d["intrinsics"], np.zeros((E, 3)), np.ones((E, 2)), d["ii"], d["jj"], d["kk"], d["bounds"])
    t3 = np.zeros((E, 3)); t3[:, :2] = e["coords"] + rng.normal(0, 0.5, (E, 2)) + target_shift
    d["targets3"] = f(t3)
    d["weights"] = d["weights_pose"] = f(rng.uniform(0.5, 1.0, (E, 2)))
    return d


CASES = {
    "one_edge": (lambda: problem([0], [1], [3], n_buf=2, p_tot=8), 1),
    "one_track": (lambda: problem([0] * 5, [1, 2, 3, 4, 5], [7] * 5, n_buf=6, p_tot=16), 1),
    "two_frames": (lambda: problem([0] * 20 + [1] * 20, [1] * 20 + [0] * 20, list(range(20)) + list(range(32, 52)), n_buf=2, p_tot=64), 1),
    "all_fixed": (lambda: problem([0] * 10 + [1] * 10, [1] * 10 + [2] * 10, list(range(10)) + list(range(16, 26)), n_buf=3, p_tot=32), 3),
    "all_masked": (lambda: problem([0] * 12, [1] * 6 + [2] * 6, list(range(6)) * 2, n_buf=3, p_tot=8, target_shift=300.0), 1),
    "self_edges": (lambda: problem([1] * 8, [1] * 8, list(range(8)), n_buf=3, p_tot=8), 1),
}


def band_120(filled):
    """120 frames of 64 tracks, each seen from the 8 frames around its source (-3 .. +4): a long thin band whose block-sparse factor
    does not fit LDS as double; filled=True sends 30 % of the observations to random frames — every block fills in (the plan is dense).
    -> ii, jj, kk, n_buf, p_tot"""
    rng = np.random.default_rng(5)
    N, M, K = 120, 64, 8                                  # (a tile of 64 tracks per frame: the band is as wide as a track's span)
    kk = np.repeat(np.arange(N * M, dtype=np.int64), K); ii = kk // M
    jj = np.clip(ii + np.tile(np.arange(K, dtype=np.int64) - 3, N * M), 0, N - 1)
    if filled:
        jj = np.where(rng.random(ii.size) < 0.3, rng.integers(0, N, ii.size), jj)
    return ii, jj, kk, N, N * M


def reprojected(g, ii, jj, kk, rng):
    """Inputs over an edge list of graphgen graph g's frames and patches: targets the reprojection of its ground truth plus 0.5 px of
    noise, weights uniform in [0.3, 1) (float32-rounded, as the caller holds them)."""
    gt = g.patches.copy(); gt[:, 2] = g.disp_gt
    u, v, _ = graphgen.reproject(g.poses_gt, gt, g.intrinsics, ii, jj, kk)
    E = len(kk)
    t3 = np.stack([u + rng.normal(0, 0.5, E), v + rng.normal(0, 0.5, E), g.disp_gt[kk]], 1)
    w = rng.uniform(0.3, 1.0, (E, 2))
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return dict(poses=f(g.poses), patches=f(g.patches), mono=f(g.mono_disp), intrinsics=f(g.intrinsics),
                targets3=f(t3), weights=f(w), weights_pose=f(w), ii=ii, jj=jj, kk=kk, bounds=np.asarray(g.bounds))


def band_120_problem(filled):
    """band_120 with frames, patches and targets of a graphgen graph of the same size -> inputs dict"""
    ii, jj, kk, N, P = band_120(filled)
    g = graphgen.make_graph(N, P // N, 8, seed=7)
    return reprojected(g, ii, jj, kk, np.random.default_rng(6))


def hub_graph(n_hubs):
    """Tracks observed from 40 frames each next to an ordinary banded graph of 48 frames (landmarks): n_hubs = 3 sit in no tile (loose
    tracks), 80 stay in tiles of 38+ cameras.  -> inputs dict, the hub tracks"""
    g = graphgen.make_graph(48, 8, 4, seed=21)
    rng = np.random.default_rng(5)
    ii, jj, kk = [g.ii], [g.jj], [g.kk]
    hub_tracks = (3, 100, 200) if n_hubs == 3 else tuple(range(2, 2 + 4 * n_hubs, 4))
    for k in hub_tracks:                                      # hub tracks: their source frame to 40 other frames
        tgt = rng.choice(48, size=40, replace=False)
        ii.append(np.full(40, k // 8)); jj.append(tgt); kk.append(np.full(40, k))
    ii, jj, kk = (np.concatenate(a).astype(np.int64) for a in (ii, jj, kk))
    return reprojected(g, ii, jj, kk, rng), hub_tracks
