"""CPU half of the world-frame point cloud / 3-D track trajectories (bt_world_tracks, include/batrack_projective.h): the
reference's fixture (tests/golden/world_tracks.npz, made by its unmodified update_point_cloud) against the numpy
restatement of the header's specification in tests/world_util.py; the ABI's refusals, the exported symbol, the operator's
schema, the CPU-tensor error and the caller's default, none of which touch a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import world_util
from batrack_amd import _lib
from batrack_amd.backend import projective_ops as pops

D = dict(np.load(world_util.GOLD))


@pytest.mark.parametrize("c", world_util.CASES)
def test_specification_reproduces_the_reference(c):
    """float64 restatement against the reference's float64 run: <= 1e-10 relative where finite, the same finiteness."""
    poses, K, pat, ix, pl, lw, m = world_util.load_case(D, c)
    points, world, out, _ = world_util.np_world_tracks(poses, K, pat, ix, pl, lw, m)
    for got, ref in ((points, D[f"{c}.points"]), (world, D[f"{c}.world"]), (out, D[f"{c}.patches_local_out"])):
        assert got.shape == ref.shape
        assert np.array_equal(np.isfinite(got), np.isfinite(ref))
        ok = np.isfinite(ref) & (ref != 0)
        assert not got[np.isfinite(ref) & (ref == 0)].any()
        err = (np.abs(got[ok] - ref[ok]) / np.abs(ref[ok])).max()
        assert err <= 1e-10, err
    assert np.array_equal(out[m:], pl[m:]) and not world[m:].any()                      # tracks past m: untouched


def test_fixture_cases_cover_what_they_claim():
    for c in world_util.CASES:
        poses, K, pat, ix, pl, lw, m = world_util.load_case(D, c)
        NM, S = pl.shape[:2]
        N, mid = poses.shape[0], (S + 1) // 2 - 1
        assert int(D[f"{c}.n"]) < N and m == int(D[f"{c}.n"]) * int(D[f"{c}.M"]) < NM    # tracks >= m exist
        live = lw[:m].sum(1) > 0
        assert 0.5 < live.mean() < 0.9
        assert (pl[:m][~live] == 0).all(-1).any() and not np.isfinite(D[f"{c}.world"][:m][~live]).all()   # never-filled slots
        j = ix[:m, None] + np.arange(S)[None] - mid
        assert (j < 0).any() and (j > N - 1).any()                                      # the clamp acts at both ends
        Xc3 = world_util.np_world_tracks(poses, K, pat, ix, pl, lw, m)[3][live]
        near = D[f"{c}.near_clamp"]
        assert near.sum() <= 0.01 * live.sum() * S                                      # at most 1 % left out
        if c == "b":
            assert (Xc3 < world_util.CLAMP).sum() > 50                                  # points behind window cameras
        else:
            assert Xc3.min() > 0.2 and not near.any()
        assert (np.ptp(K, axis=0) > 0).all() == (c == "c")                              # intrinsics differ between frames
        for k in ("points", "world", "disp"):
            assert 0 < float(D[f"gate.{c}.{k}"]) < 1e-4
        # the reference's own float32 run: the finiteness of its float64 run, and the clamp decided the same way
        assert np.array_equal(np.isfinite(D[f"{c}.world32"]), np.isfinite(D[f"{c}.world"]))
        o32, o64 = D[f"{c}.patches_local_out32"][:m][live], D[f"{c}.patches_local_out"][:m][live]
        keep = ~near[live]
        assert world_util.uv_err(o32[..., :2][keep], o64[..., :2][keep])[0] < 2e-5


def test_symbol_is_exported_and_operator_registered():
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bt_world_tracks")
    ops = _lib.torch_ops(strict=True)
    s = str(ops.world_tracks.default._schema)
    assert s.startswith("batrack_hip::world_tracks(Tensor poses, Tensor patches, Tensor intrinsics, Tensor ix, Tensor(a!) patches_local, "
                        "Tensor local_weights, int m, Tensor(b!)? points=None, Tensor(c!)? world=None)")
    assert "bt_world_tracks" in open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "batrack_projective.h")).read()
    assert "world_tracks.hip" in _lib.SOURCES


def test_abi_refuses_before_launching():
    """Argument checks return their codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    p = ctypes.c_void_p(256)                           # never dereferenced: every call below is refused first
    ok = dict(poses=p, N=4, K=p, pat=p, NM=8, pe=1, ix=p, pl=p, lw=p, S=3, m=8, points=p, world=p)
    call = lambda **k: L.bt_world_tracks(*(dict(ok, **k)[n] for n in ok), None)
    for name in ("poses", "K", "pat", "ix", "pl", "lw"):
        assert call(**{name: None}) == _lib.BT_EINVAL, name
    assert call(m=9) == _lib.BT_EINVAL                 # m > N*M
    assert call(m=-1) == _lib.BT_EINVAL
    assert call(S=0) == _lib.BT_EINVAL
    assert call(pe=0) == _lib.BT_EINVAL
    assert call(pe=8) == _lib.BT_EINVAL                # not a p x p patch
    assert call(N=0) == _lib.BT_EINVAL
    assert call(S=(1 << 20) + 1) == _lib.BT_EUNSUPPORTED
    assert call(m=0) == _lib.BT_OK                     # nothing to do, nothing launched


def test_cpu_tensors_raise():
    N, M, S = 3, 2, 3
    a = (torch.zeros(1, N, 7), torch.zeros(1, N * M, 3, 1, 1), torch.ones(1, N, 4), torch.zeros(N * M, dtype=torch.int64),
         torch.zeros(1, N * M, S, 3), torch.zeros(1, N * M, S, 1))
    with pytest.raises(RuntimeError, match="GPU"):
        pops.world_tracks(*a, N * M)
    with pytest.raises(RuntimeError, match="GPU"):
        _lib.torch_ops(strict=True).world_tracks(a[0][0], a[1][0], a[2][0], a[3], a[4][0], a[5][0, ..., 0], N * M)


def test_point_cloud_step_is_off_by_default():
    from batrack_amd.sequence import SlamConfig, SyntheticObservations, WindowedBA
    assert SlamConfig().UPDATE_POINT_CLOUD is False
    obs = SyntheticObservations(n_frames=4, M=8)
    w = WindowedBA(obs, ba=None)
    assert not hasattr(w, "trajs_3d_world_") and not hasattr(w, "points_")
    cfg = SlamConfig(PATCHES_PER_FRAME=8, BUFFER_SIZE=5, UPDATE_POINT_CLOUD=True)
    w = WindowedBA(obs, ba=None, cfg=cfg)
    assert w.trajs_3d_world_.shape == (5, 8, w.S_local, 3) and w.points_.shape == (40, 3)


INPUT_KEYS = ("poses", "intrinsics", "patches", "ix", "patches_local", "local_weights")


def _sha(d):
    import hashlib
    h = hashlib.sha256()
    for k in INPUT_KEYS:
        h.update(np.ascontiguousarray(d[k]).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("args,seed,sha", [
    ((51, 256, 12, 50), 307, "aefaad1c7fa71aa307178e79544f5fb2449c319b3a87d7dd30763828b2685382"),
    ((12, 16, 4, 11), 5, "9680e07ac24658a8c4e0544265ad961bb0d140145abd145a7bf18f35487b378d")])
def test_random_inputs_defaults_are_unchanged(args, seed, sha):
    """The arrays random_inputs gave before it took `S_local=` and `p=` (their sha256, recorded then), bit for bit; the new
    arguments at the values the defaults stand for give the same arrays, and `p=` changes the patches alone."""
    d = world_util.random_inputs(*args, seed=seed)
    assert _sha(d) == sha and d["m"] == args[3] * args[1]
    assert d["patches"].shape == (args[0] * args[1], 3, 1, 1) and d["patches_local"].shape[1] == 2 * args[2] - 1
    same = world_util.random_inputs(*args, seed=seed, S_local=2 * args[2] - 1)
    assert _sha(same) == sha
    p3 = world_util.random_inputs(*args, seed=seed, p=3)
    assert all(np.array_equal(p3[k], d[k]) for k in INPUT_KEYS if k != "patches")
    assert np.array_equal(p3["patches"][:, :, 1, 1], d["patches"][:, :, 0, 0])
    even = world_util.random_inputs(*args, seed=seed, S_local=8)
    assert even["patches_local"].shape == (args[0] * args[1], 8, 3) and even["local_weights"].shape == (args[0] * args[1], 8)
    assert all(np.array_equal(even[k], d[k]) for k in ("poses", "intrinsics", "patches", "ix"))


@pytest.mark.parametrize("p", [2, 3, 64])
def test_specification_picks_the_centre_of_decoy_filled_patches(p):
    """Every pixel but (p/2, p/2) of the p x p patches is a decoy in +-1000: the restatement's result equals the p = 1
    result bit for bit, in float32 and in float64, and a neighbouring pixel taken for the centre moves it by far more than
    any gate."""
    one = world_util.random_inputs(12, 16, 4, 11, seed=5)
    dec = world_util.random_inputs(12, 16, 4, 11, seed=5, p=p)
    assert dec["patches"].shape == (192, 3, p, p)
    off = np.ones((p, p), bool)
    off[p // 2, p // 2] = False
    assert np.abs(dec["patches"][..., off]).max() > 900 and (np.abs(dec["patches"][..., off]) > 1.5).mean() > 0.99
    for dt in (np.float32, np.float64):
        run = lambda d: world_util.np_world_tracks(*(d[k] if k == "ix" else d[k].astype(dt) for k in INPUT_KEYS), d["m"])[:3]
        a, b = run(one), run(dec)
        assert all(x.dtype == dt and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
        wrong = dict(dec, patches=np.roll(dec["patches"], 1, axis=-1))          # the pixel left of the centre in its place
        assert world_util.rel_err(run(wrong)[0], a[0].astype(np.float64)) > 0.1     # the measure saturates near 1; gates are ~1e-6
