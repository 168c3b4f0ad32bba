"""The step between the tracker and the BA inside the caller's loop: a 24-frame WindowedBA replay (M = 8, S_slam = 4) run
once with `observer` = the HIP op (batrack_amd.frontend.observe.window_observations) and once with the torch restatement
(tests/observe_util.window_observations_ref), same BA, same device.  After EVERY frame the edges' targets and weights,
patches_valid_ and the window buffers of the two runs are equal bit for bit."""
import numpy as np
import pytest
import torch

import observe_util as ou

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATE = ("targets_3d", "weights", "weights_pose", "patches_valid_", "patches_monodisp_", "patches_local_", "patches_local_monodisp_",
         "patches_local_vis_", "patches_local_static_", "patches_local_weights_")


def test_replay_with_the_op_equals_the_replay_with_the_restatement():
    from batrack_amd import graphgen
    from batrack_amd.backend.ba import BA_rgbd_droid
    from batrack_amd.frontend.observe import window_observations
    from batrack_amd.sequence import SlamConfig, SyntheticObservations, WindowedBA
    cam = dict(graphgen.SINTEL, wd=256, ht=112, cx=128.0, cy=56.0, fx=125.0, fy=125.0)
    n_frames, M = 24, 8
    runs = []
    for observer in (window_observations, ou.window_observations_ref):
        obs = SyntheticObservations(n_frames=n_frames, M=M, seed=4, cam=cam)
        cfg = SlamConfig(PATCHES_PER_FRAME=M, BUFFER_SIZE=n_frames + 1, num_init=6, init_updates=4, ITER=2, OPTIMIZATION_WINDOW=8,
                         REMOVAL_WINDOW=10, S_slam=4)
        runs.append(WindowedBA(obs, BA_rgbd_droid, cfg, device=DEV, observer=observer))
    seen = dict(edges=0, weights=0, pose=0, valid=0)
    for f in range(n_frames):
        for trk in runs:
            trk()
        a, b = runs
        assert a.n == b.n == f + 1 and torch.equal(a.kk, b.kk) and torch.equal(a.jj, b.jj)
        for k in STATE:
            assert ou.same_bits(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()), f"frame {f}: {k} differs"
        assert ou.same_bits(a.poses_.cpu().numpy(), b.poses_.cpu().numpy()), f"frame {f}: poses differ"
        seen["edges"] = max(seen["edges"], a.kk.numel())
    a = runs[0]
    seen.update(weights=int((a.weights > 0).sum()), pose=int((a.weights_pose > 0).sum()), valid=int((a.patches_valid_ > 0).sum()))
    # the replay did something: edges with weight, fewer of them for the poses (moving tracks), valid tracks, a moved camera
    assert seen["edges"] > 0 and 0 < seen["pose"] < seen["weights"] and seen["valid"] > 0
    assert float(a.patches_monodisp_.abs().sum()) > 0 and float(a.poses_[1:a.n, :3].abs().sum()) > 0
    assert bool(torch.isfinite(a.poses_).all())


def test_default_replay_is_untouched():
    """observer=None: the host path, no new buffers."""
    from batrack_amd.sequence import SyntheticObservations, WindowedBA
    w = WindowedBA(SyntheticObservations(n_frames=4, M=8), ba=None)
    assert w.observer is None and not hasattr(w, "patches_monodisp_") and not hasattr(w, "patches_local_monodisp_")
