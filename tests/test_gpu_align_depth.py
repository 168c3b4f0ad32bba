"""-m gpu: the depth-map alignment of the dense global-alignment stage (main/global_refine/model/utils.py:268-312) on the HIP
kernels (bt_align_depth_maps, include/batrack_depth.h), bit for bit:
  against the unmodified reference's outputs (tests/golden/align_depth.npz), and against the host restatement
  `_align_depth_maps` at the Sintel size (50 x 436 x 1024, float64 and float32) and for T = 1 and T = 2;
  numpy and tensor input, in place, a repeated call; `scales` / `overlap` against the host's branch decisions;
  RefineLosses.from_results(align_depth=True) against the host-aligned path on ga_init.npz and on a WindowedBA result;
  the tensor call enqueues without synchronising.
Every comparison is exact (NaN where the reference has NaN; the other elements' bits)."""
import os

import numpy as np
import pytest
import torch

from align_util import host_align_stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = dict(np.load(os.path.join(ROOT, "tests", "golden", "align_depth.npz")))
NAMES = [str(n) for n in D["names"]]
DEV = "cuda:0"


def assert_same(out, ref):
    """Exactly equal: NaN at the same places, the bits of every other element equal (so -0 and +0 differ)."""
    out, ref = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (out, ref))
    assert out.dtype == ref.dtype and out.shape == ref.shape
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(out), nan)
    u = f"u{ref.dtype.itemsize}"
    np.testing.assert_array_equal(np.ascontiguousarray(out[~nan]).view(u), np.ascontiguousarray(ref[~nan]).view(u))


def host(maps):
    from batrack_amd.global_refine import _align_depth_maps
    with np.errstate(all="ignore"):
        return _align_depth_maps(maps)


def sintel_scene(dtype, T=50, H=436, W=1024, seed=0):
    """A mono-depth-like scene: smooth positive depth, a per-frame scale drift, invalid (0) and negative pixels, a frame with
    almost no valid pixels (skipped) and one right after it."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = 2.0 + 8.0 * (0.5 + 0.5 * np.sin(3 * x + 2 * y))
    maps = np.empty((T, H, W, 1), np.float64)
    for t in range(T):
        d = base * rng.uniform(0.5, 2.0) * (1 + 0.1 * rng.standard_normal((H, W)))
        d[rng.random((H, W)) < 0.03] = 0.0
        d[rng.random((H, W)) < 0.001] = -1.0
        maps[t, ..., 0] = d
    maps[T // 2, 8:] = 0.0                                                # 8 rows of 1024: overlap >= 100 still
    maps[T // 2 + 4, :, W // 2:] = 0.0                                    # left half, then right half: no overlap, skipped;
    maps[T // 2 + 5, :, :W // 2] = 0.0                                    # the frame after it has an empty past set
    return maps.astype(dtype)


# ---------------------------------------------------------------------- the reference's fixture
@pytest.mark.parametrize("name", NAMES)
def test_numpy_input_matches_the_reference_fixture(name, capsys):
    from batrack_amd.global_refine import align_depth_maps
    maps, ref = D[f"{name}.maps"], D[f"{name}.aligned"]
    out, scales, overlap = align_depth_maps(maps, return_stats=True)
    assert_same(out, ref)
    printed = capsys.readouterr().out
    want = "".join(f"Insufficient overlapping region found between depth map {i - 1} and {i} ({c} pixels). Using previous transformation.\n"
                   for i, c in zip(D[f"{name}.skipped"], D[f"{name}.printed"]))
    assert printed == want
    _, hs, ho, _ = host_align_stats(maps[..., 0])
    np.testing.assert_array_equal(overlap, ho)
    np.testing.assert_array_equal(scales, hs)


@pytest.mark.parametrize("name", NAMES)
def test_tensor_input_in_place_and_repeat_match_the_fixture(name):
    from batrack_amd.global_refine import align_depth_maps, align_depth_maps_device
    maps, ref = D[f"{name}.maps"], D[f"{name}.aligned"]
    x = torch.as_tensor(maps, device=DEV)
    out, scales, overlap = align_depth_maps(x, return_stats=True)
    assert out.is_cuda and out.shape == x.shape and out.dtype == x.dtype
    assert_same(out, ref)
    out3 = align_depth_maps(x[..., 0])                                    # [T,H,W]
    assert_same(out3, ref[..., 0])
    again = align_depth_maps(x)
    np.testing.assert_array_equal(again.cpu().numpy().view(f"u{ref.dtype.itemsize}"), out.cpu().numpy().view(f"u{ref.dtype.itemsize}"))
    ch0 = x[..., 0].contiguous()
    a, s, o = align_depth_maps_device(ch0, out=ch0)                       # in place
    assert a.data_ptr() == ch0.data_ptr()
    assert_same(ch0, ref[..., 0])
    assert torch.equal(o, overlap)
    np.testing.assert_array_equal(s.cpu().numpy(), scales.cpu().numpy())


# ---------------------------------------------------------------------- against the host restatement
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sintel_size_matches_the_host_bit_for_bit(dtype):
    from batrack_amd.global_refine import align_depth_maps
    maps = sintel_scene(dtype)
    ref = host(maps)
    x = torch.as_tensor(maps[..., 0], device=DEV)
    out, scales, overlap = align_depth_maps(x, return_stats=True)
    assert torch.equal(out, torch.as_tensor(ref[..., 0], device=DEV))
    _, hs, ho, _ = host_align_stats(maps[..., 0])
    np.testing.assert_array_equal(overlap.cpu().numpy(), ho)
    np.testing.assert_array_equal(scales.cpu().numpy(), hs)
    assert (ho[1:] < 100).sum() == 1 and np.isnan(hs[1:]).sum() == 1     # one skipped frame, the rest scaled
    out_np = align_depth_maps(maps)                                       # numpy in: the same
    assert_same(out_np, ref)
    from batrack_amd.global_refine import align_depth_maps_device
    x4 = torch.as_tensor(maps, device=DEV)
    v = x4.view(maps.shape[0], -1)
    align_depth_maps_device(v, out=v)                                     # in place, [T, hw]
    assert torch.equal(x4, torch.as_tensor(ref, device=DEV))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", [1, 2])
def test_one_and_two_frames(T, dtype):
    from batrack_amd.global_refine import align_depth_maps
    rng = np.random.default_rng(T)
    maps = rng.uniform(0.5, 4.0, (T, 37, 29, 2)).astype(dtype)          # hw = 1073: not a multiple of 16 bytes (scalar loads)
    maps[..., 0][rng.random((T, 37, 29)) < 0.2] = 0.0
    ref = host(maps)
    out, scales, overlap = align_depth_maps(maps, return_stats=True)
    assert_same(out, ref)
    _, hs, ho, _ = host_align_stats(maps[..., 0])
    np.testing.assert_array_equal(overlap, ho)
    np.testing.assert_array_equal(scales, hs)
    if T == 1:
        assert_same(out, maps)


# ---------------------------------------------------------------------- from_results
def _check_from_results(res, **kw):
    from batrack_amd.global_refine import RefineLosses
    dm = np.asarray(res["dmaps"])
    hres = dict(res)
    hres["dmaps"] = host(dm)                                              # what from_results aligned on the host before
    dev = RefineLosses.from_results(dict(res), DEV, align_depth=True, **kw)
    ref = RefineLosses.from_results(hres, DEV, align_depth=False, **kw)
    assert torch.equal(dev.dmaps, ref.dmaps)
    assert torch.equal(dev.trajs_disp_mono, ref.trajs_disp_mono)
    a, b = dev.get_results()["dmaps"], ref.get_results()["dmaps"]
    assert a.dtype == b.dtype == dm.dtype
    np.testing.assert_array_equal(a, b)
    return dev


def test_from_results_on_the_ga_init_fixture_is_the_host_path_bit_for_bit():
    G = dict(np.load(os.path.join(ROOT, "tests", "golden", "ga_init.npz"), allow_pickle=False))
    res = {k[3:]: v for k, v in G.items() if k.startswith("in.")}
    res.update(rgbs=None, dmaps_gt=None)
    weights = dict(zip(("spatial_loss", "inter_frame_loss", "pts_3d_loss", "cam_smooth_vec_loss", "scale_smoothness_loss"),
                       (float(x) for x in G["weights"])))
    for dt in (np.float64, np.float32):
        r = dict(res, dmaps=np.asarray(res["dmaps"]).astype(dt))
        _check_from_results(r, grid_size=4, loss_weight_dict=weights, refine_intrinsics=True)


def test_from_results_on_a_windowed_ba_result_is_the_host_path_bit_for_bit():
    from batrack_amd import graphgen
    from batrack_amd.backend.ba import BA_rgbd_droid
    from batrack_amd.sequence import SlamConfig, SyntheticObservations, WindowedBA
    cam = dict(graphgen.SINTEL, wd=256, ht=112, cx=128.0, cy=56.0, fx=125.0, fy=125.0)
    n_frames, M = 12, 48
    obs = SyntheticObservations(n_frames=n_frames, M=M, seed=5, cam=cam)
    cfg = SlamConfig(PATCHES_PER_FRAME=M, BUFFER_SIZE=n_frames + 1, num_init=6, init_updates=6, ITER=2, OPTIMIZATION_WINDOW=8,
                     REMOVAL_WINDOW=10, S_slam=6)
    trk = WindowedBA(obs, BA_rgbd_droid, cfg, device=DEV)
    trk.run()
    rng = np.random.default_rng(2)
    mono = [obs.depth_map(f) * rng.uniform(0.7, 1.4) * (1 + 0.05 * rng.standard_normal(obs.depth_map(f).shape)) for f in range(n_frames)]
    res = trk.get_results(dmaps=mono)
    assert res["dmaps"].dtype == np.float64
    net = _check_from_results(res, grid_size=12, loss_weight_dict={"spatial_loss": 5.0, "inter_frame_loss": 0.3, "pts_3d_loss": 1.0})
    assert np.isfinite(float(net.loss()))


# ---------------------------------------------------------------------- no synchronisation
def test_tensor_call_does_not_synchronise():
    from batrack_amd.global_refine import align_depth_maps
    maps = torch.as_tensor(sintel_scene(np.float64, T=12, H=64, W=96), device=DEV)
    align_depth_maps(maps)                                                # load the code objects, fill the allocator's cache
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                                  # the mode is live on this build
        out, scales, overlap = align_depth_maps(maps, return_stats=True)
        out3 = align_depth_maps(maps[..., 0])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    ref = host(maps.cpu().numpy())
    assert torch.equal(out, torch.as_tensor(ref, device=DEV)) and torch.equal(out3, torch.as_tensor(ref[..., 0], device=DEV))
