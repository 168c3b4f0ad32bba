"""bt_world_tracks on the GPU (include/batrack_projective.h): the fused kernel against the reference's float64 run of its
unmodified update_point_cloud (tests/golden/world_tracks.npz), against the same computation composed from the operations
the package had before it, and through the replayed caller with `UPDATE_POINT_CLOUD`.

Gates.  (u, v) of patches_local: the project's gate for fused reprojection, |got - ref| / (100 + |ref|) < 2e-5 where
|ref| < 1e4 (tests/test_gpu_projective.py:45-49).  Disparity column, points and world: the reference's own float32 run
against its float64 run, e32 = max |ref32 - ref64| / (1 + |ref64|), is stored in the fixture as gate.*; the kernel must stay
within 2 x e32 — a fused kernel composes the two group actions in another order than the reference's separate calls and is
not held to less rounding than the reference's own float32 path shows.  Finiteness must agree exactly."""
import numpy as np
import pytest
import torch

import world_util as wu
from batrack_amd.backend import projective_ops as pops
from batrack_amd.backend.lietorch import SE3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = dict(np.load(wu.GOLD))
UV_GATE = 2e-5
np64 = lambda t: t.detach().cpu().numpy().astype(np.float64)


def _flat(points, world, out):
    return np64(points), np64(world)[0], np64(out)[0]


@pytest.mark.parametrize("c", wu.CASES)
def test_fused_matches_the_reference_fixture(c):
    d = wu.fixture_case(D, c)
    m = int(d["m"])
    got = _flat(*wu.run_fused(wu.to_gpu(d, DEV)))
    ref = (D[f"{c}.points"], D[f"{c}.world"], D[f"{c}.patches_local_out"])
    live = d["local_weights"][:m].sum(1) > 0
    f = wu.parity_figures(got, ref, m, live, D[f"{c}.near_clamp"])
    e32 = {k: float(D[f"gate.{c}.{k}"]) for k in ("points", "world", "disp")}
    msg = f"case {c}: kernel {f}, e32 {e32}"
    print(msg)
    assert f["finite"], msg
    assert f["rest"], msg                                        # not-live tracks and tracks >= m: patches_local bit-equal
    assert not got[1][m:].any(), msg                             # world rows past m: not written
    # (share of the (u, v) entries with |ref| < 1e4: in case b the clamp multiplies the 27 % of entries behind a camera by 100)
    assert f["uv"] < UV_GATE and f["uv_share"] > (0.7 if c == "b" else 0.9), msg
    for k in ("points", "world", "disp"):
        assert f[k] <= 2.0 * e32[k], msg


@pytest.mark.parametrize("N,M,S_slam,n", [(51, 256, 12, 50), (1024, 256, 12, 1023)])
def test_fused_equals_composed_operations(N, M, S_slam, n):
    """A user's size (12,800 tracks, 294,400 slots) and the full buffer (261,888 tracks: 4,092 blocks of 64 tracks, past one
    pass of the grid of at most 2,048 workgroups); the composed result as the reference, the fixture's case (a) e32 for the outputs without a
    project gate; untouched tracks bit-equal; two calls bit-equal."""
    d = wu.random_inputs(N, M, S_slam, n, seed=N + M)
    g = wu.to_gpu(d, DEV)
    m = g["m"]
    a = wu.run_fused(g)
    b = wu.run_fused(g)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))      # bit for bit, NaN included
    ref = wu.composed_world_tracks(SE3, g["poses"], g["patches"], g["intrinsics"], g["ix"], g["patches_local"],
                                   g["local_weights"], m)
    assert torch.equal(a[2][0, m:], g["patches_local"][0, m:]) and torch.equal(a[1][0, m:], torch.zeros_like(a[1][0, m:]))
    live = d["local_weights"][:m].sum(1) > 0
    assert 0.6 < live.mean() < 0.8
    f = wu.parity_figures(_flat(*a), _flat(*ref), m, live)
    e32 = {k: float(D[f"gate.a.{k}"]) for k in ("points", "world", "disp")}
    msg = f"N {N} M {M} S_slam {S_slam} m {m}: fused against composed {f}, e32 of case a {e32}"
    print(msg)
    assert f["finite"] and f["rest"], msg
    assert f["uv"] < UV_GATE and f["uv_share"] > 0.9, msg
    for k in ("points", "world", "disp"):
        assert f[k] <= 2.0 * e32[k], msg


def test_bad_source_frame_and_views():
    """An ix outside [0, N) gives NaN for that track alone; SE3 / tensor poses, [N, M, ...] buffers and caller-owned outputs."""
    d = wu.fixture_case(D, "a")
    g = wu.to_gpu(d, DEV)
    m, S = g["m"], g["patches_local"].shape[2]
    live = (g["local_weights"][:m].sum(1) > 0).cpu().numpy()
    kl, kn = int(np.flatnonzero(live)[0]), int(np.flatnonzero(~live)[0])
    good = wu.run_fused(g)
    bad = dict(g, ix=g["ix"].clone())
    bad["ix"][kl], bad["ix"][kn] = g["poses"].shape[1], -1
    p, w, pl = wu.run_fused(bad)
    for k in (kl, kn):
        assert bool(torch.isnan(p[k]).all()) and bool(torch.isnan(w[0, k]).all())
    assert bool(torch.isnan(pl[0, kl]).all()) and torch.equal(pl[0, kn], g["patches_local"][0, kn])
    others = torch.ones(m, dtype=torch.bool, device=DEV)
    others[[kl, kn]] = False
    eq = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert eq(p[others], good[0][others]) and eq(w[0, :m][others], good[1][0, :m][others]) and eq(pl[0, :m][others], good[2][0, :m][others])
    # the caller's buffers: [N, M, S_local, 3] views, SE3 poses, outputs it owns
    N, M = g["poses"].shape[1], int(D["a.M"])
    plc = g["patches_local"].clone().view(N, M, S, 3)
    points_, world_ = torch.full((N * M, 3), 7.0, device=DEV), torch.full((N, M, S, 3), 7.0, device=DEV)
    p2, w2 = pops.world_tracks(SE3(g["poses"]), g["patches"], g["intrinsics"], g["ix"], plc, g["local_weights"].view(N, M, S, 1), m,
                               points=points_, world=world_)
    assert p2.data_ptr() == points_.data_ptr() and w2.data_ptr() == world_.data_ptr() and w2.shape == (1, N * M, S, 3)
    assert eq(p2, good[0]) and eq(w2[0, :m], good[1][0, :m]) and eq(plc.view(1, N * M, S, 3), good[2])
    assert bool((points_[m:] == 7.0).all()) and bool((world_.view(N * M, S, 3)[m:] == 7.0).all())
    with pytest.raises(RuntimeError, match="contiguous"):
        pops.world_tracks(g["poses"], g["patches"], g["intrinsics"], g["ix"], g["patches_local"][:, ::2], g["local_weights"], m)


def test_through_the_caller():
    """24 frames of the replayed caller with UPDATE_POINT_CLOUD against a subclass that composes the step from the older
    operations after each update(): final poses within 1e-5 (the gate of two runs of the same kernels,
    test_windowed_ba_through_the_reference_names); after the last update the depth prior of every live track,
    patches_local_[:, :, mid, 2], is its current disparity patches_[:, :, 2] up to rounding — the feedback the reference has
    and the default replay lacks."""
    f = wu.caller_feedback(DEV)
    msg = f"caller: {f}"
    print(msg)
    assert f["pose_diff"] < 1e-5, msg
    assert f["live"] > 100, msg
    assert f["dev_fused"] <= 2.0 * f["dev_composed"] and f["dev_fused"] < 1e-5, msg
    assert f["dev_default"] > 1e-3, msg                          # without the step the prior stays the tracker's disparity
    assert f["keys"] == 11 and f["trajs_2d_disp_is_buffer"], msg
    assert f["points_finite"] and f["world_rows_written"] == f["m"], msg
