"""-m gpu: the dense global-alignment losses and their gradients (include/batrack_ga.h) at the limits their kernels enforce or
rely on, against the float64 oracles (oracle/ga_losses.py, oracle/ga_torch.py):
  - tracks per frame at every LDS boundary of the two pairwise kernels (N = 3968 .. 4096 = BT_GA_MAX_TRACKS), and N = 4097
    refused before anything is enqueued (sentinel-filled outputs stay untouched);
  - track positions off the image (the scale grid's zero padding), on its last row / column and on cell boundaries;
  - scale grids that are not 4x4: non-square, one cell wide or high (an empty smoothness direction), and 12 * 1024 cells,
    the backward's limit (one more is refused); the smoothness term in all three modes.
Gates: 1e-5 on the losses and the total, 5e-5 on every gradient relative to its largest entry, as
test_gpu_global_refine.test_total_and_every_gradient_match_the_reference."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_global_refine as G  # noqa: E402

from oracle import ga_losses as ga  # noqa: E402
from oracle import ga_torch  # noqa: E402

pytestmark = pytest.mark.gpu

W_RUN = [G.RUN_WEIGHTS[k] for k in ("spatial_loss", "inter_frame_loss", "pts_3d_loss", "cam_smooth_vec_loss", "scale_smoothness_loss")]
SMOOTH = {"l1": 0, "l2": 1, "huber": 2}
SENTINEL = -12345.0


def backward_total(net, w, mode):
    """bt_ga_backward_total with the smoothness mode given (RefineLosses.backward always takes forward()'s 'l1')."""
    from batrack_amd import _lib
    net._run(1)                                                               # mono_scaled for the current parameters
    ms = net._mono_scaled
    g = {k: torch.empty(shape, device=ms.device, dtype=torch.float32) for k, shape in
         (("g_ms", ms.shape), ("trajs_scales", ms.shape), ("frame_scales_", net.frame_scales_.shape), ("pose", (net.T, 7)), ("intrinsics", (net.T, 4)))}
    a = net._args(0)
    st = torch.cuda.current_stream(ms.device).cuda_stream
    _lib.check(net._lib.bt_ga_backward_total(ctypes.byref(a), ms.data_ptr(), ctypes.byref(_lib.GaWeights(*w, SMOOTH[mode])), g["g_ms"].data_ptr(),
                                             g["trajs_scales"].data_ptr(), g["frame_scales_"].data_ptr(), g["pose"].data_ptr(),
                                             g["intrinsics"].data_ptr(), st), "bt_ga_backward_total")
    g["K"] = g["intrinsics"].sum(0) * net.K_scale
    return g


def check_case(d, mode="l1", w=W_RUN, desc=""):
    """Every loss, the weighted total and the gradients w.r.t. trajs_scales, frame_scales_, pose and K (the intrinsics refined,
    as run_global_refine.py runs it).  Returns the largest errors."""
    net = G.build(d, **dict(G._settings("A"), scale_smoothness_weight=w[4]))
    d_k = dict(d, intrinsics=net.intrinsics.cpu().numpy().astype(np.float64))  # K * K_scale as the kernels read it
    l = net.losses(mode).cpu().numpy()
    ms = ga.frame_scaled_depth(d_k)
    errs = {}
    for got, want, name in zip(l, (ga.spatial_loss(d_k, ms), ga.inter_frame_loss(d_k, ms), ga.pts_3d_loss(d_k, ms)), ("spatial", "rigid", "pts3d")):
        errs[name] = abs(got - want) / abs(want)
        assert abs(got - want) <= 1e-5 * abs(want), (desc, name, got, want)
    r = ga_torch.full_total_and_grads(d, w, mode, refine_intrinsics=True)
    for i, name in enumerate(("spatial", "rigid", "pts3d", "cam_smooth", "scale_smooth")):
        assert abs(l[i] - r[name]) <= 1e-5 * abs(r[name]) + 1e-12, (desc, name, l[i], r[name])
    tot = sum(wi * l[i] for i, wi in enumerate(w))
    assert abs(tot - r["total"]) <= 1e-5 * abs(r["total"]), (desc, tot, r["total"])
    g = backward_total(net, w, mode)
    for k, key in (("trajs_scales", "grad_trajs_scales"), ("frame_scales_", "grad_frame_scales"), ("pose", "grad_pose"), ("K", "grad_K")):
        got, ref = g[k].cpu().numpy().astype(np.float64), np.asarray(r[key])
        assert np.isfinite(got).all(), (desc, k)
        if np.abs(ref).max() == 0:
            assert np.abs(got).max() == 0.0, (desc, k)
            errs[k] = 0.0
        else:
            errs[k] = G._gerr(got, ref)
            assert errs[k] < 5e-5, (desc, k, errs[k])
    print(desc, mode, " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    return errs


# ------------------------------------------------------------------ tracks per frame at the LDS boundaries
# forward: M * 80 B of LDS, M = (N + 1) / 2; backward: ceil(M / 64) * 64 * 80 B, 163,840 B (all a workgroup has) from N = 3969
@pytest.mark.parametrize("N", [3968, 3969, 4094, 4095, 4096])
def test_tracks_per_frame_at_the_lds_limit(N):
    d = G.make_case(3, N, 3, seed=N)
    d["grid_query_frames"] = np.array([1], np.int64)                          # the frame whose every slot is in the window
    check_case(d, desc=f"N={N}")


def _sentinel_like(t, dtype=None):
    return torch.full(t.shape if hasattr(t, "shape") else t, SENTINEL, device="cuda:0", dtype=dtype or torch.float32)


def _refusal_case(N, gh=4, gw=4):
    d = G.make_case(2, N, 3, seed=7)
    d["grid_query_frames"] = np.array([0, 1], np.int64)
    return G.build(G.regrid(d, gh, gw, seed=7), **G._settings("A"))


def _forward_raw(net, which):
    from batrack_amd import _lib
    ms, losses = _sentinel_like(net._mono_scaled), _sentinel_like((5,), torch.float64)
    a = net._args(0)
    rc = net._lib.bt_ga_forward(ctypes.byref(a), ms.data_ptr(), losses.data_ptr(), which, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, ms, losses, _lib


def _backward_raw(net, w):
    from batrack_amd import _lib
    ms = net._mono_scaled
    outs = [_sentinel_like(ms), _sentinel_like(ms), _sentinel_like(net.frame_scales_), _sentinel_like((net.T, 7)), _sentinel_like((net.T, 4))]
    a = net._args(0)
    rc = net._lib.bt_ga_backward_total(ctypes.byref(a), ms.data_ptr(), ctypes.byref(_lib.GaWeights(*w, 0)), *[o.data_ptr() for o in outs],
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, outs, _lib


def test_one_track_past_the_limit_is_refused_before_anything_is_enqueued():
    net = _refusal_case(4097)
    net._mono_scaled.fill_(0.5)
    for which in (3, 15, 2 | 8):
        rc, ms, losses, _lib = _forward_raw(net, which)
        assert rc == _lib.BT_EUNSUPPORTED, (which, rc)
        assert bool((ms == SENTINEL).all()) and bool((losses == SENTINEL).all()), which
    rc, outs, _lib = _backward_raw(net, W_RUN)
    assert rc == _lib.BT_EUNSUPPORTED, rc
    assert all(bool((o == SENTINEL).all()) for o in outs)
    with pytest.raises(RuntimeError, match="4096 tracks per frame"):
        net.losses()


def test_the_terms_without_the_pairwise_kernels_take_any_number_of_tracks():
    """The limit is the inter-frame term's: the others run at N = 4097 and match the oracle."""
    net = _refusal_case(4097)
    net._run(1)                                                               # mono_scaled for the backward
    rc, ms, losses, _lib = _forward_raw(net, 1 | 4 | 8)
    assert rc == _lib.BT_OK, rc
    d = G.make_case(2, 4097, 3, seed=7)
    d = dict(G.regrid(d, 4, 4, seed=7), grid_query_frames=np.array([0, 1], np.int64))
    d_k = dict(d, intrinsics=net.intrinsics.cpu().numpy().astype(np.float64))
    ref_ms = ga.frame_scaled_depth(d_k)
    assert np.abs(ms.cpu().numpy() - ref_ms).max() < 2e-6 * np.abs(ref_ms).max()
    l = losses.cpu().numpy()
    assert abs(l[0] / ga.spatial_loss(d_k, ref_ms) - 1) < 1e-5 and abs(l[2] / ga.pts_3d_loss(d_k, ref_ms) - 1) < 1e-5 and l[1] == 0.0
    w = [5.0, 0.0, 1.0, 1.0, 0.3]
    rc, outs, _lib = _backward_raw(net, w)
    assert rc == _lib.BT_OK, rc
    r = ga_torch.full_total_and_grads(d, w, "l1", refine_intrinsics=True)
    for o, key in zip(outs[1:3], ("grad_trajs_scales", "grad_frame_scales")):
        assert G._gerr(o.cpu().numpy(), r[key]) < 5e-5, key


def test_a_grid_past_the_backward_limit_is_refused_before_anything_is_enqueued():
    net = _refusal_case(300, 1, 12 * 1024 + 1)
    net._run(1)
    rc, outs, _lib = _backward_raw(net, W_RUN)
    assert rc == _lib.BT_EUNSUPPORTED, rc
    assert all(bool((o == SENTINEL).all()) for o in outs)


# ------------------------------------------------------------------ positions off the image, other grids, every smoothness mode
@pytest.mark.parametrize("mode", ["l1", "l2", "huber"])
@pytest.mark.parametrize("gh,gw", [(4, 4), (3, 7), (6, 2), (1, 5), (5, 1), (1, 1), (12, 1024)])
def test_positions_off_the_image_and_other_grids(gh, gw, mode):
    d = G.make_case(5, 301, 5, seed=gh * 100 + gw)
    d["grid_query_frames"] = np.array([1, 2, 4], np.int64)
    d = G.move_outside(G.regrid(d, gh, gw, seed=gh + gw, spread=6.0), 0.3, seed=gh * gw)
    xy = d["trajs_2d"]
    H, W = int(d["H"]), int(d["W"])
    # every kind of position is there
    assert (xy[..., 0] < 0).any() and (xy[..., 1] < 0).any() and (xy[..., 0] > W - 1).any() and (xy[..., 1] > H - 1).any()
    assert (xy[..., 0] == W - 1).any() and (xy[..., 1] == H - 1).any()
    check_case(d, mode, desc=f"grid {gh}x{gw}")
