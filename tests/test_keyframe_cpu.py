"""Motion-magnitude keyframe removal, CPU side: the torch restatement in `WindowedBA.keyframe()` against the fixture made
from the reference's `BATRACK.keyframe` (tests/golden/keyframe.npz), the observation model's slot -> frame translation,
a replay in which frames really leave the buffer, and the C ABI's argument checks (no GPU call is made by any of them)."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import keyframe_util as ku
from batrack_amd import _lib, evaluation
from batrack_amd.sequence import SlamConfig, SyntheticObservations, WindowedBA
from oracle.se3_torch import SE3Ref
from sequence_util import oracle_BA_rgbd_droid
from test_sequence import small_cfg

# The restatement's two magnitudes against the fixture's: both are float32 torch evaluations on the CPU.  Measured on the six
# cases (magnitudes of 9.4 - 14.7 px): |restatement - fixture| = 0 in every case — the restatement issues the same torch
# operations in the same order as the reference, the SE3 formulas included, so there is no summation-order difference to
# allow for.  Twice the measured error is allowed: none.
MAG_TOL = 2 * 0.0


@pytest.fixture(scope="module")
def golden():
    return np.load(ku.GOLDEN)


@pytest.mark.parametrize("case", ku.CASES)
def test_restatement_reproduces_the_fixture(golden, case):
    d = ku.load_case(case, golden)
    t = ku.tracker_from_case(d, se3=SE3Ref)
    k = int(d["n_in"]) - int(d["KEYFRAME_INDEX"])
    mags = [t.motionmag(i, k) if bool(((t.ii == i) & (t.jj == k)).any()) else float("nan") for i in (k - 1, k + 1)]
    t.keyframe()
    assert t.n == int(d["n_out"]) and t.m == int(d["m_out"])
    for k in ("ii", "jj", "kk"):
        assert np.array_equal(getattr(t, k).numpy(), d[k + "_out"]), k
    for k in ("targets_3d", "weights", "weights_pose"):
        assert np.array_equal(getattr(t, k)[0].numpy(), d[k + "_out"]), k
    for name in ku.BUFFERS:
        if name != "colors":
            assert np.array_equal(getattr(t, name + "_").numpy(), d[name + "_out"]), name
    assert t.tstamps[:t.n] == [int(x) for x in d["tstamps_out"][:t.n]]
    decided = case != "e"
    assert len(t.keyframe_log) == (1 if decided else 0)
    if decided:
        removed = t.keyframe_log[0][2]
        assert removed == bool(d["removed"])
        err = np.abs(np.array(mags) - d["mags"])
        print(f"case {case}: magnitudes {mags} fixture {d['mags']} |difference| {err}")
        assert np.array_equal(np.isnan(mags), np.isnan(d["mags"]))
        assert np.nanmax(err, initial=0.0) <= MAG_TOL
    # delta: the removed time stamp -> (the one before it, their relative pose)
    assert sorted(t.delta) == sorted(int(x) for x in d["delta_t"][:, 0])
    for (t1, t0), dP in zip(d["delta_t"], d["delta_dP"]):
        assert t.delta[int(t1)][0] == int(t0)
        assert np.abs(t.delta[int(t1)][1].data.numpy().reshape(7) - dP).max() < 1e-6


def window_edges(M, n=9, Sp=6):
    lo = n - Sp
    q = (np.arange(lo, n, 2)[:, None] * M + np.arange(M)[None]).reshape(-1)
    return np.repeat(q, Sp), np.tile(np.arange(lo, n), q.size)


def obs_digest(obs, M, **kw):
    kk, jj = window_edges(M)
    h = hashlib.sha256()
    for a in obs.predict(kk, jj, **kw):
        h.update(np.ascontiguousarray(a).tobytes())
    for a in obs.predict_window(kk, jj, 8, **kw):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


# sha256 over predict + predict_window of the commit before `slot_frame` existed, on the sequences of test_sequence.py
PARENT_DIGESTS = {(24, 4, 3): "a1571ba8a62ff19f", (22, 24, 5): "969c1cd283ce3cff", (14, 8, 7): "003d8aaeed137ec5"}


@pytest.mark.parametrize("n_frames,M,seed", sorted(PARENT_DIGESTS))
def test_slot_frame_none_and_identity_change_nothing(n_frames, M, seed):
    mk = lambda: SyntheticObservations(n_frames=n_frames, M=M, seed=seed)
    assert obs_digest(mk(), M) == PARENT_DIGESTS[(n_frames, M, seed)]
    assert obs_digest(mk(), M, slot_frame=None) == PARENT_DIGESTS[(n_frames, M, seed)]
    assert obs_digest(mk(), M, slot_frame=np.arange(n_frames)) == PARENT_DIGESTS[(n_frames, M, seed)]


def test_slot_frame_translates_tracks_and_frames():
    """After the removal of frame 4, slot s >= 4 holds frame s + 1: the edges (slot track -> slot frame) are the source edges."""
    M = 4
    sf = np.array([0, 1, 2, 3, 5, 6, 7, 8, 9, 10])
    kk, jj = window_edges(M)
    a = SyntheticObservations(n_frames=12, M=M, seed=3).predict(kk, jj, slot_frame=sf)
    b = SyntheticObservations(n_frames=12, M=M, seed=3).predict(sf[kk // M] * M + kk % M, sf[jj])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    wa = SyntheticObservations(n_frames=12, M=M, seed=3).predict_window(kk, jj, 6, slot_frame=sf)
    wb = SyntheticObservations(n_frames=12, M=M, seed=3).predict_window(kk, jj, 6)
    assert np.array_equal(wa[4][..., 0], wb[4][..., 0])                     # the query's frame in the window: slot numbers
    assert not np.array_equal(wa[4][..., 1:], wb[4][..., 1:])               # its position: the source track's


# Candidates' m/2 on this sequence with the threshold below (CPU, oracle BA): removed 3.411, 3.276, 3.315, 3.495; the
# closest kept ones 3.849, 3.853, 3.875.  The threshold sits in the middle of the gap (0.175 px on either side).
REPLAY = dict(n_frames=26, M=16, seed=5)
REPLAY_CFG = dict(kf_stride=1, use_keyframe=True, KEYFRAME_INDEX=4, KEYFRAME_THRESH=3.67)


def check_replay_conditions(trk, obs):
    log = trk.keyframe_log
    removed = [t for t, _, r in log if r]
    assert len(removed) >= 3 and sum(not r for _, _, r in log) >= 3, log
    assert min(abs(m - trk.cfg.KEYFRAME_THRESH) for _, m, _ in log) >= 0.05, log
    assert sorted(trk.delta) == removed and trk.n == obs.n_frames - len(removed) and trk.m == trk.n * obs.M
    return removed


def test_replay_with_removed_keyframes():
    obs = SyntheticObservations(**REPLAY)
    trk = WindowedBA(obs, oracle_BA_rgbd_droid, small_cfg(obs, **REPLAY_CFG), se3=SE3Ref)
    for _ in range(obs.n_frames):
        trk()
        E = trk.ii.numel()
        assert bool((trk.ii == trk.kk // obs.M).all())
        assert trk.jj.numel() == trk.kk.numel() == E
        assert trk.targets_3d.shape == (1, E, 3) and trk.weights.shape == (1, E, 2) and trk.weights_pose.shape == (1, E, 2)
        assert E == 0 or (int(trk.jj.max()) < trk.n and int(trk.ii.max()) < trk.n)
        assert trk.tstamps[:trk.n] == trk.tstamps_[:trk.n].tolist() == sorted(set(range(trk.counter)) - set(trk.delta))
    removed = check_replay_conditions(trk, obs)
    print("removed time stamps", removed, "log", [(t, round(m, 3), r) for t, m, r in trk.keyframe_log])
    poses, tstamps = trk.terminate()
    assert poses.shape == (obs.n_frames, 7) and tstamps.tolist() == list(range(obs.n_frames))
    assert np.abs(np.linalg.norm(poses[:, 3:], axis=1) - 1.0).max() < 1e-5
    gt = obs.centres_gt()
    ate = evaluation.ate_rmse(poses[:, :3].astype(np.float64), gt)
    still = evaluation.ate_rmse(np.zeros_like(gt) + 1e-9 * np.arange(gt.shape[0])[:, None], gt)
    assert ate < 0.25 * still and ate < 0.005, (ate, still)          # the bound of test_oracle_driven_sequence_tracks_the_camera
    # the hand-off: one pose per time stamp, the buffer's for the frames still in it
    T = trk.get_results()["cams_T_world"]
    assert T.shape == (obs.n_frames, 4, 4) and np.abs(T[:, :3, 3] - poses[:, :3]).max() < 1e-6
    kept = [t for t in range(obs.n_frames) if t not in trk.delta]
    assert np.abs(T[kept][:, :3, 3] - evaluation.camera_centres(trk.poses_[:trk.n].numpy().astype(np.float64))).max() < 1e-5


def test_default_config_never_calls_keyframe():
    obs = SyntheticObservations(n_frames=14, M=8, seed=7)
    trk = WindowedBA(obs, lambda Gs, patches, *a, **k: (Gs, patches), small_cfg(obs, USE_MAP_FILTERING=False), se3=SE3Ref)
    trk.run()
    assert not SlamConfig().use_keyframe and trk.keyframe_log == [] and trk.delta == {} and trk.n == trk.counter == 14
    poses, tstamps = trk.terminate()
    assert np.abs(SE3Ref(torch.as_tensor(poses[:, [0, 1, 2, 4, 5, 6, 3]])).inv().data.numpy() - trk.poses_[:14].numpy()).max() < 1e-6


def test_keyframe_symbols_are_exported():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("bt_keyframe_workspace_bytes", "bt_edges_prune_tile", "bt_edges_prune_scan_span", "bt_keyframe_decide",
                 "bt_edges_prune", "bt_rows_shift"):
        assert hasattr(L, name), name
    L = _lib.lib()
    tile, span = L.bt_edges_prune_tile(), L.bt_edges_prune_scan_span()
    assert tile >= 64 and tile % 64 == 0 and span >= 1 and tile * (span + 1) + 3 <= 4 << 20
    assert ctypes.sizeof(_lib.KeyframeStatus) == 32
    assert L.bt_keyframe_workspace_bytes(0) >= 32 and L.bt_keyframe_workspace_bytes(10 * tile) >= L.bt_keyframe_workspace_bytes(0) + 40


def test_argument_errors_return_codes():
    """Every check returns before anything is enqueued: the pointers below are never dereferenced (no GPU here)."""
    L = _lib.lib()
    EINVAL, EUNS = _lib.BT_EINVAL, _lib.BT_EUNSUPPORTED
    p = lambda i: 0x10000 * i                                    # distinct, aligned, 64 KiB apart
    ws = p(40)
    good = [p(1), p(2), p(3)]
    dec = lambda k=3, idx=good, E=100, ws=ws, pe=1, n_poses=8: L.bt_keyframe_decide(k, *idx, E, p(4), n_poses, p(5), 64, pe, p(6), 0.5, 10.0, ws, None)
    assert dec(ws=None) == EINVAL and dec(E=-1) == EINVAL and dec(k=-2) == EINVAL and dec(idx=[None, p(2), p(3)]) == EINVAL
    assert dec(pe=2) == EINVAL and dec(pe=0) == EINVAL and dec(n_poses=-1) == EINVAL and dec(E=2 ** 31) == EUNS
    ins, outs = [p(i) for i in range(1, 7)], [p(i) for i in range(11, 17)]
    prune = lambda E=100, M=8, ins=ins, outs=outs, ws=ws: L.bt_edges_prune(3, 10, M, 5, *ins, E, *outs, ws, None)
    assert prune(ws=None) == EINVAL and prune(E=-1) == EINVAL and prune(M=0) == EINVAL and prune(E=2 ** 31) == EUNS
    assert prune(ins=[None] + ins[1:]) == EINVAL and prune(outs=outs[:5] + [None]) == EINVAL
    assert prune(outs=[ins[0]] + outs[1:]) == EINVAL                           # in place
    assert prune(outs=[ins[1] + 8 * 99] + outs[1:]) == EINVAL                  # the last row of an input
    assert prune(outs=[outs[1]] + outs[1:]) == EINVAL                          # two outputs alike
    assert prune(outs=outs[:3] + [ins[5] - 12 * 100 + 4] + outs[4:]) == EINVAL  # ends one float into an input
    assert prune(outs=[ws] + outs[1:]) == EINVAL                               # the workspace
    assert prune(outs=[outs[0] + 4] + outs[1:]) == EINVAL                      # misaligned
    bufs = (_lib.RowBuffer * 17)(*[_lib.RowBuffer(p(20 + i), 4) for i in range(17)])
    shift = lambda nbuf=2, k=3, n=10, bufs=bufs, ws=ws: L.bt_rows_shift(bufs, nbuf, k, n, ws, None)
    assert shift(nbuf=17) == EINVAL and shift(nbuf=-1) == EINVAL and shift(ws=None) == EINVAL and shift(bufs=None) == EINVAL
    assert shift(k=-1) == EINVAL and shift(nbuf=0, k=-1) == _lib.BT_OK
    bad = (_lib.RowBuffer * 2)(_lib.RowBuffer(p(20), 4), _lib.RowBuffer(p(21), 0))
    assert shift(bufs=bad) == EINVAL
    bad[1] = _lib.RowBuffer(None, 4)
    assert shift(bufs=bad) == EINVAL
    assert shift(k=9, n=10) == _lib.BT_OK and shift(k=12, n=10) == _lib.BT_OK   # nothing to move: nothing enqueued


def test_prune_keyframe_refuses_cpu_tensors():
    from batrack_amd.frontend.keyframe import prune_keyframe
    z = torch.zeros
    with pytest.raises(RuntimeError, match="GPU"):
        prune_keyframe(z(4, 7), z(8, 3, 1, 1), z(4, 4), z(2, dtype=torch.int64), z(2, dtype=torch.int64), z(2, dtype=torch.int64),
                       z(1, 2, 3), z(1, 2, 2), z(1, 2, 2), n=4, M=2, kf_stride=1)
