"""Test-side helpers for the keyframe removal (tests/golden/keyframe.npz, made by tests/golden/make_golden_keyframe.py): the
fixture's names, a `WindowedBA` filled from a fixture case, and numpy statements of the three stages of
include/batrack_keyframe.h.  Test infrastructure only."""
import os

import numpy as np
import torch

CASES = ("a", "b", "c", "d", "e", "f")
EDGES = ("ii", "jj", "kk", "targets_3d", "weights", "weights_pose")
# the eleven buffers the reference shifts (batrack.py:1052-1063), by their attribute names without the trailing underscore
BUFFERS = ("tstamps", "colors", "poses", "patches", "intrinsics", "patches_local", "patches_local_vis", "patches_local_static",
           "patches_local_weights", "patches_valid", "trajs_3d_world")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe.npz")


def load_case(c, z=None):
    z = z if z is not None else np.load(GOLDEN)
    return {k[len(c) + 1:]: z[k] for k in z.files if k.startswith(c + ".")}


def tracker_from_case(d, device="cpu", se3=None, keyframer=None):
    """A WindowedBA in the fixture's state before the call (no __init__: it needs an observation model)."""
    from batrack_amd.sequence import SlamConfig, WindowedBA
    t = object.__new__(WindowedBA)
    t.cfg = SlamConfig(PATCHES_PER_FRAME=int(d["M"]), kf_stride=int(d["kf_stride"]), KEYFRAME_INDEX=int(d["KEYFRAME_INDEX"]),
                       KEYFRAME_THRESH=float(d["KEYFRAME_THRESH"]), REMOVAL_WINDOW=int(d["REMOVAL_WINDOW"]), use_keyframe=True)
    t.device = torch.device(device)
    t.SE3, t.keyframer = se3, keyframer
    t.N, t.M, t.n, t.m = d["poses_in"].shape[0], int(d["M"]), int(d["n_in"]), int(d["m_in"])
    for name in BUFFERS:
        if name != "colors":                                    # the project keeps no colour buffer
            setattr(t, name + "_", torch.as_tensor(d[name + "_in"].copy(), device=device))
    t.tstamps = [int(x) for x in d["tstamps_in"]]
    t.ii, t.jj, t.kk = (torch.as_tensor(d[k + "_in"].copy(), device=device) for k in ("ii", "jj", "kk"))
    t.targets_3d, t.weights, t.weights_pose = (torch.as_tensor(d[k + "_in"].copy(), device=device)[None]
                                               for k in ("targets_3d", "weights", "weights_pose"))
    t.delta, t.keyframe_log = {}, []
    return t


def np_prune(ii, jj, kk, removed, k, n, M, window):
    """(keep mask, ii', jj', kk') of bt_edges_prune, as the boolean masks of batrack.py:1045-1050, 1072."""
    ii, jj, kk = ii.copy(), jj.copy(), kk.copy()
    keep = np.ones(ii.shape, bool)
    if removed:
        keep &= ~((ii == k) | (jj == k))
        kk[ii > k] -= M
        ii[ii > k] -= 1
        jj[jj > k] -= 1
        n = n - 1
    keep &= ~(kk // M < n - window)
    return keep, ii[keep], jj[keep], kk[keep]


def flow_mag64(poses, patches, intrinsics, ii, jj, kk, beta=0.5):
    """The reference's flow_mag at the centre pixel in float64 torch arithmetic (projective_ops.py:112-122 over the oracle's
    SE3 formulas): what both the parent's float32 evaluation and the kernel are measured against."""
    from batrack_amd.backend import projective_ops as pops
    from oracle.se3_torch import SE3Ref
    P = SE3Ref(torch.as_tensor(poses, dtype=torch.float64).reshape(1, -1, 7))
    pat = torch.as_tensor(patches, dtype=torch.float64)
    pat = pat.reshape(1, -1, *pat.shape[-3:])
    K = torch.as_tensor(intrinsics, dtype=torch.float64).reshape(1, -1, 4)
    c = pat.shape[-1] // 2
    f = pops.flow_mag(P, pat, K, torch.as_tensor(ii), torch.as_tensor(jj), torch.as_tensor(kk), beta=beta)
    return f[0, :, c, c]


def mean_flow64(poses, patches, intrinsics, ii, jj, kk, i, j, beta=0.5):
    sel = (ii == i) & (jj == j)
    if not sel.any():
        return float("nan")
    return float(flow_mag64(poses, patches, intrinsics, ii[sel], jj[sel], kk[sel], beta).mean())
