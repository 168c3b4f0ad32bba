"""Motion-magnitude keyframe removal on the device: `prune_keyframe` (batrack_amd/frontend/keyframe.py over
csrc/keyframe.hip) on every case of the fixture made from the reference's `BATRACK.keyframe`, the replay with frames
leaving the buffer against its CPU / oracle twin, and the default path with and without the keyframer."""
import numpy as np
import pytest
import torch

import keyframe_util as ku
from batrack_amd import evaluation
from batrack_amd.sequence import SyntheticObservations, WindowedBA
from oracle.se3_torch import SE3Ref
from sequence_util import oracle_BA_rgbd_droid
from test_keyframe_cpu import REPLAY, REPLAY_CFG, check_replay_conditions
from test_sequence import small_cfg

pytestmark = pytest.mark.gpu

# The two magnitudes against a float64 torch evaluation of flow_mag on the same inputs (keyframe_util.mean_flow64).  The
# yardstick is the error of the formulation this replaces, the fused float32 `pops.flow_mag(...).mean()` on the device,
# against that same float64 value.  Measured on the fixture's pairs on an MI355X (profiles/r15_keyframe.txt): the parent's
# largest error is 4.37e-6 px, at the pair (11 -> 10), 9.402 px (4.6e-7 relative; the per-edge float32 arithmetic, which
# the kernel shares: its mean is the same float32 number there); its other pairs show 0.9e-6 and 1.4e-6 px, the kernel's
# 1.9e-6 px (the next float32 number: the kernel adds in double and rounds once).  The kernel may show twice the
# parent's largest.
PARENT_MAG_ERR_PX = 4.37e-6
MAG_TOL_PX = 2 * PARENT_MAG_ERR_PX


@pytest.fixture(scope="module")
def golden():
    return np.load(ku.GOLDEN)


def parent_mean_flow(d, i, j, dev="cuda:0"):
    """The parent's formulation: boolean-mask gather, fused float32 reprojections, .mean().item()."""
    from batrack_amd.backend import projective_ops as pops
    from batrack_amd.backend.lietorch import SE3
    up = lambda a: torch.as_tensor(a, device=dev)
    ii, jj, kk = up(d["ii_in"]), up(d["jj_in"]), up(d["kk_in"])
    sel = (ii == i) & (jj == j)
    P = up(d["poses_in"])[None]
    pat = up(d["patches_in"]).reshape(1, -1, 3, 1, 1)
    return pops.flow_mag(SE3(P), pat, up(d["intrinsics_in"])[None], ii[sel], jj[sel], kk[sel], beta=0.5).mean().item()


@pytest.mark.parametrize("case", ku.CASES)
def test_fixture_through_the_kernels(golden, case):
    from batrack_amd.frontend.keyframe import KeyframeConfig, prune_keyframe
    d = ku.load_case(case, golden)
    dev = "cuda:0"
    up = lambda a: torch.as_tensor(a.copy(), device=dev)
    bufs = {name: up(d[name + "_in"]) for name in ku.BUFFERS}
    edges = {k: up(d[k + "_in"]) for k in ku.EDGES}
    n, M = int(d["n_in"]), int(d["M"])
    cfg = KeyframeConfig(KEYFRAME_INDEX=int(d["KEYFRAME_INDEX"]), KEYFRAME_THRESH=float(d["KEYFRAME_THRESH"]),
                         REMOVAL_WINDOW=int(d["REMOVAL_WINDOW"]))
    r = prune_keyframe(bufs["poses"], bufs["patches"].view(-1, 3, 1, 1), bufs["intrinsics"], edges["ii"], edges["jj"], edges["kk"],
                       edges["targets_3d"][None], edges["weights"][None], edges["weights_pose"][None], n=n, M=M,
                       kf_stride=int(d["kf_stride"]), cfg=cfg, frame_buffers=[bufs[name] for name in ku.BUFFERS])
    assert r.removed == bool(d["removed"]) and r.k == n - cfg.KEYFRAME_INDEX
    for k, got in (("ii", r.ii), ("jj", r.jj), ("kk", r.kk), ("targets_3d", r.targets_3d[0]), ("weights", r.weights[0]),
                   ("weights_pose", r.weights_pose[0])):
        assert np.array_equal(got.cpu().numpy(), d[k + "_out"]), k
    for name in ku.BUFFERS:                                      # all eleven, the colours' uint8 rows included
        assert np.array_equal(bufs[name].cpu().numpy(), d[name + "_out"]), name
    for k in ku.EDGES:                                           # out of place: the inputs are as they were
        assert np.array_equal(edges[k].cpu().numpy(), d[k + "_in"]), k
    if case == "e":
        assert r.ii is edges["ii"] and r.dP is None and np.isnan(r.mag_prev) and np.isnan(r.mag_next)
        return
    k = r.k
    want = [ku.mean_flow64(d["poses_in"], d["patches_in"], d["intrinsics_in"], d["ii_in"], d["jj_in"], d["kk_in"], i, k) for i in (k - 1, k + 1)]
    got = [r.mag_prev, r.mag_next]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(got), np.isnan(d["mags"]))
    for g, w, i in zip(got, want, (k - 1, k + 1)):
        if not np.isnan(w):
            par = parent_mean_flow(d, i, k)
            print(f"case {case} pair ({i} -> {k}): float64 {w!r} kernel {g!r} off by {abs(g - w):.3e} px; parent's float32 {par!r} off by {abs(par - w):.3e} px")
            assert abs(g - w) <= MAG_TOL_PX, (g, w)
    if r.removed:
        assert np.abs(r.dP.cpu().numpy() - d["delta_dP"][0]).max() < 1e-6
    else:
        assert r.dP is None


@pytest.fixture(scope="module")
def replays():
    from batrack_amd.backend.ba import BA_rgbd_droid
    from batrack_amd.frontend.keyframe import prune_keyframe
    out = {}
    for name, ba, dev, kw in (("hip", BA_rgbd_droid, "cuda:0", dict(keyframer=prune_keyframe)),
                              ("oracle", oracle_BA_rgbd_droid, "cpu", dict(se3=SE3Ref))):
        obs = SyntheticObservations(**REPLAY)
        trk = WindowedBA(obs, ba, small_cfg(obs, **REPLAY_CFG), device=dev, **kw)
        trk.run()
        removed = check_replay_conditions(trk, obs)
        poses, _ = trk.terminate()
        out[name] = dict(trk=trk, removed=removed, poses=poses,
                         ate=evaluation.ate_rmse(poses[:, :3].astype(np.float64), obs.centres_gt()))
    return out


def test_replay_matches_the_cpu_replay(replays):
    h, o = replays["hip"], replays["oracle"]
    assert h["removed"] == o["removed"], (h["trk"].keyframe_log, o["trk"].keyframe_log)
    for k in ("ii", "jj", "kk"):
        assert np.array_equal(getattr(h["trk"], k).cpu().numpy(), getattr(o["trk"], k).numpy()), k
    assert h["trk"].n == o["trk"].n and h["trk"].tstamps == o["trk"].tstamps
    assert h["trk"].tstamps_[:h["trk"].n].tolist() == h["trk"].tstamps[:h["trk"].n]
    assert h["poses"].shape == o["poses"].shape == (REPLAY["n_frames"], 7)
    assert abs(h["ate"] - o["ate"]) <= 0.01 * o["ate"], (h["ate"], o["ate"])


def test_default_path_is_unchanged_by_the_keyframer():
    """use_keyframe off: `keyframe_simple` through the device pipeline leaves, frame by frame, the list the boolean mask leaves."""
    from batrack_amd.backend.ba import BA_rgbd_droid
    from batrack_amd.frontend.keyframe import prune_keyframe
    trks = []
    for kw in (dict(), dict(keyframer=prune_keyframe)):
        obs = SyntheticObservations(n_frames=24, M=32, seed=2)
        trks.append(WindowedBA(obs, BA_rgbd_droid, small_cfg(obs), device="cuda:0", **kw))
    for f in range(24):
        for t in trks:
            t()
        a, b = trks
        for k in ("ii", "jj", "kk", "targets_3d"):               # (the weights pass through map filtering: the BA's atomics)
            assert torch.equal(getattr(a, k), getattr(b, k)), (f, k)
        assert a.weights.shape == b.weights.shape and a.weights_pose.shape == b.weights_pose.shape
    assert a.n == b.n == 24 and b.delta == {} and b.keyframe_log == []
    assert int(a.ii.min()) >= a.n - a.cfg.REMOVAL_WINDOW          # the window did remove edges
