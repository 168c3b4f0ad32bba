"""-m gpu: the mono-depth alignment (main/mono_depth/get_mono_depth.py:21-150) on the HIP kernels (bt_mono_align,
include/batrack_depth.h), exactly:
  every case of the unmodified reference's fixture (tests/golden/mono_depth.npz) through align_mono_depth and through the
  file-level align_depth; random scenes of T in {1, 2, 3, 17, 64} frames of 1 .. 777 pixels in both dtypes, with ties and
  non-finite values, and one DAVIS-size scene (50 x 480 x 854, past 2^24 elements), against the numpy restatement
  (mono_util.py) including its intermediates; repeated calls and a workspace full of 0xFF give the same bits; a call on a side
  stream enqueues without synchronising.
Equality is np.array_equal(..., equal_nan=True) with equal dtypes."""
import os

import numpy as np
import pytest
import torch

from mono_util import restate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = dict(np.load(os.path.join(ROOT, "tests", "golden", "mono_depth.npz")))
CASES = [str(n) for n in D["names"]]
DEV = "cuda:0"


def same(out, ref):
    out, ref = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (out, ref))
    assert out.dtype == ref.dtype and out.shape == ref.shape, (out.dtype, ref.dtype, out.shape, ref.shape)
    assert np.array_equal(out, ref, equal_nan=True), np.flatnonzero(~((out == ref) | (np.isnan(out) & np.isnan(ref))))[:10]


def bits(x):
    a = x.detach().cpu().numpy()
    return a.view(f"u{a.dtype.itemsize}")


def check_against_numpy(d, m, **kw):
    from batrack_amd.mono_depth import align_mono_depth
    out, s, c, al, k = align_mono_depth(torch.as_tensor(d, device=DEV), torch.as_tensor(m, device=DEV), return_stats=True, **kw)
    depth, rs, rc, ral, rk = restate(d, m)
    same(s, rs)
    same(c, rc)
    assert k == rk
    same(al, ral)
    same(out, depth)
    return out


def pairs(case):
    d, m = D[f"{case}.mono"], D[f"{case}.metric"]
    T = min(len(d), len(m))
    return d[:T], m[:T]


# ---------------------------------------------------------------------- the reference's fixture
@pytest.mark.parametrize("case", CASES)
def test_golden_case_through_align_mono_depth(case):
    out = check_against_numpy(*pairs(case))
    same(out, D[f"{case}.depth"])


@pytest.mark.parametrize("case", CASES)
def test_golden_case_through_the_file_level_align_depth(case, tmp_path, capsys):
    from PIL import Image
    from batrack_amd.mono_depth import align_depth
    names = [str(n) for n in D[f"{case}.names"]]
    mono_root, metric_root, img_dir = tmp_path / "mono", tmp_path / "metric", tmp_path / "images" / case
    for p in (mono_root / case, metric_root / case, img_dir):
        p.mkdir(parents=True)
    for name, x in zip(names, D[f"{case}.mono"]):
        np.save(mono_root / case / (name + ".npy"), x)
    for name, x, k in zip(names, D[f"{case}.metric"], D[f"{case}.intrinsics"]):
        np.savez(metric_root / case / (name + ".npz"), depth=x, intrinsics=k)
    h, w = D[f"{case}.image_hw"].tolist()
    Image.new("RGB", (w, h)).save(img_dir / "00000.png")
    out_d, out_k = tmp_path / "out" / case, tmp_path / "out_K" / case
    align_depth(str(mono_root), str(metric_root), case, str(img_dir), str(out_d), str(out_k))
    n = len(D[f"{case}.depth"])
    assert sorted(os.listdir(out_d)) == [x + ".npy" for x in names[:n]]
    assert sorted(os.listdir(out_k)) == [x + "_intrinsics.npy" for x in names[:n]]
    for t, name in enumerate(names[:n]):
        same(np.load(out_d / (name + ".npy")), D[f"{case}.depth"][t])
        K = np.load(out_k / (name + "_intrinsics.npy"))
        assert K.dtype == np.float64 and np.array_equal(K.view(np.uint64), D[f"{case}.K"].view(np.uint64))
    warned = "WARNING: Mismatch in number of depth files! Mono: 5, Metric: 4" in capsys.readouterr().out
    assert warned == (case == "mismatch")


# ---------------------------------------------------------------------- random scenes against the restatement
def random_scene(seed, T, hw, dt):
    rng = np.random.default_rng(1000 + seed)
    d = rng.choice(np.linspace(0.0, 1.0, 23, dtype=np.float32), (T, 1, hw))             # ties
    d = np.where(rng.random(d.shape) < 0.5, rng.random(d.shape, np.float32), d).astype(np.float32)
    d[rng.random(d.shape) < 0.05] = np.float32(0.02)
    m = (1.0 / (rng.uniform(0.5, 2.0, (T, 1, 1)) * d + rng.uniform(0.01, 0.2, (T, 1, 1)))).astype(dt)
    m[rng.random(m.shape) < 0.1] = dt(2.0)
    m[rng.random(m.shape) < 0.02] = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, -3.0, -1e-8], dt))
    if T > 1 and seed % 4 == 1:
        m[1 + seed % (T - 1), 0, rng.integers(hw)] = np.nan                            # a metric frame other than 0
    if seed % 7 == 3:
        d[rng.integers(T), 0, rng.integers(hw)] = np.nan                                # mono: all NaN out
    return d, m


@pytest.mark.parametrize("seed", range(40))
def test_random_scene_matches_numpy(seed):
    T = (1, 2, 3, 17, 64)[seed % 5]
    hw = (1, 2, 3, 777, 768)[(seed // 5) % 5]
    dt = (np.float64, np.float32)[seed % 2]
    check_against_numpy(*random_scene(seed, T, hw, dt))


def davis_scene(T=50, H=480, W=854, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, H, dtype=np.float32), np.linspace(0, 1, W, dtype=np.float32), indexing="ij")
    d = np.empty((T, H, W), np.float32)
    m = np.empty((T, H, W), np.float32)
    for t in range(T):
        base = 0.02 + 0.9 * (0.5 + 0.5 * np.sin(2.5 * x + 1.5 * y + 0.1 * t))
        d[t] = base * (1 + np.float32(0.05) * rng.standard_normal((H, W), np.float32))
        m[t] = 1 / (np.float32(rng.uniform(0.5, 2)) * d[t] + np.float32(0.05)) * (1 + np.float32(0.03) * rng.standard_normal((H, W), np.float32))
    return d, m


def test_davis_size_past_2_to_the_24_matches_numpy():
    d, m = davis_scene()
    assert d.size > 1 << 24
    check_against_numpy(d, m)


# ---------------------------------------------------------------------- repeatability and streams
def _raw_call(d, m, ws_fill=None):
    from batrack_amd import _lib
    L = _lib.lib()
    T, hw = d.shape[0], d[0].numel()
    dt = _lib.BT_DEPTH_F64 if m.dtype == torch.float64 else _lib.BT_DEPTH_F32
    ws = torch.empty(int(L.bt_mono_align_workspace_bytes(T, hw, dt)), dtype=torch.uint8, device=DEV)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    out, fs, fc = torch.empty_like(m), torch.empty(T, dtype=m.dtype, device=DEV), torch.empty(T, dtype=m.dtype, device=DEV)
    al, k = torch.empty(3, dtype=m.dtype, device=DEV), torch.empty(1, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.bt_mono_align(d.data_ptr(), m.data_ptr(), T, hw, dt, out.data_ptr(), fs.data_ptr(), fc.data_ptr(), al.data_ptr(),
                               k.data_ptr(), ws.data_ptr(), st), "bt_mono_align")
    return out, fs, fc, al, k


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_repeated_calls_and_a_dirty_workspace_give_the_same_bits(dt):
    d, m = random_scene(5, 17, 777, dt)
    d, m = torch.as_tensor(d, device=DEV), torch.as_tensor(m, device=DEV)
    first = _raw_call(d, m)
    for fill in (None, 0xFF, None):
        again = _raw_call(d, m, fill)
        for a, b in zip(first, again):
            assert np.array_equal(bits(a), bits(b))
    from batrack_amd.mono_depth import align_mono_depth
    out = torch.full_like(m, float("nan"))
    assert align_mono_depth(d, m, out=out) is out
    assert np.array_equal(bits(out), bits(first[0]))


def test_side_stream_call_does_not_synchronise():
    from batrack_amd.mono_depth import align_mono_depth
    d, m = random_scene(2, 17, 768, np.float32)
    dg, mg = torch.as_tensor(d, device=DEV), torch.as_tensor(m, device=DEV)
    align_mono_depth(dg, mg)                                                  # load the code objects, fill the allocator's cache
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                                      # the mode is live on this build
        with torch.cuda.stream(side):
            out = align_mono_depth(dg, mg)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    side.synchronize()
    same(out, restate(d, m)[0])
