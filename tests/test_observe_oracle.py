"""CPU half of the window observations (bt_observe_window, include/batrack_observe.h): the torch restatement
tests/observe_util.window_observations_ref against the fixture tests/golden/observe_window.npz, which the reference's
unmodified predict_target made (tests/golden/make_golden_observe.py) — every output and every buffer bit for bit, no
tolerance: the step is comparisons, selects, a subtraction, a correctly rounded division and the interpolation.  And the
restatement's quantile against torch.quantile, bit for bit, over random sizes and q."""
import ctypes
import os

import numpy as np
import pytest
import torch

import observe_util as ou

@pytest.fixture(scope="module")
def gold():
    return np.load(ou.GOLD)


@pytest.mark.parametrize("case", ou.CASES)
def test_restatement_equals_the_reference_bit_for_bit(gold, case):
    args, kw, want = ou.load_case(gold, case)
    got = ou.results(ou.window_observations_ref(*args, **kw), kw)
    for k in ou.OUTPUTS:
        assert ou.same_bits(got[k], want[k]), f"case {case}: {k} differs from the reference's"


@pytest.mark.parametrize("case", ou.CASES)
def test_fixture_leaves_untouched_what_the_reference_leaves(gold, case):
    """The fixture itself: rows of patches_valid outside the window's keyframes and slots no edge names keep their input."""
    g = lambda k: gold[f"{case}.{k}"]
    n, Sp, kf = int(g("n")), int(g("Sp")), int(g("kf_stride"))
    rows = np.zeros(g("patches_valid_in").shape[0], bool)
    rows[n - Sp:n:kf] = True
    assert np.array_equal(g("patches_valid_out")[~rows], g("patches_valid_in")[~rows])
    S_local = g("local_vis_in").shape[1]
    slot = g("jj") - g("ii") + (S_local + 1) // 2 - 1
    ok = (slot >= 0) & (slot < S_local)
    hit = np.zeros(g("local_vis_in").shape, bool)
    hit[g("kk")[ok], slot[ok]] = True
    assert hit.sum() == ok.sum()                      # no (kk, slot) pair twice
    for b in ou.BUFFERS:
        assert ou.same_bits(g(b + "_out")[~hit], g(b + "_in")[~hit]), b
        assert not ou.same_bits(g(b + "_out")[hit], g(b + "_in")[hit]), b


def test_fixture_holds_the_cases_it_names(gold):
    g = lambda c, k: gold[f"{c}.{k}"]
    th = {c: ou.static_threshold(torch.as_tensor(g(c, "dyn")), float(g(c, "STATIC_QUANTILE")), float(g(c, "STATIC_THRESHOLD")))
          for c in ou.CASES}
    assert th["c_below"] < ou.f32(0.1) and th["c_above"] == ou.f32(0.1) and np.isnan(th["e"])
    assert int(g("b", "Sp")) < g("b", "traj").shape[0] and int(g("b", "n")) < int(g("b", "MIN_TRACK_LEN")) and not g("b", "is_initialized")
    assert ou.same_bits(g("b", "patches_valid_out"), g("b", "patches_valid_in"))      # both validity rules off
    assert not g("e", "weights_pose").any() and g("e", "weights").any()
    d = "d_len"
    assert th[d] < ou.f32(0.1) and ((1 - g(d, "dyn")) == np.float32(th[d])).sum() >= 2                    # scores equal to the threshold
    x, y = g(d, "targets_3d")[:, 0], g(d, "targets_3d")[:, 1]
    for v, a in ((20.0, x), (44.0, x), (20.0, y), (float(g(d, "ht")) - 20.0, y)):
        assert (a == np.float32(v)).any()                                                                 # coordinates exactly at the bounds
    assert (g(d, "vis") == np.float32(0.9)).any()
    assert np.isnan(g(d, "targets_3d")[:, 2]).any() and np.isnan(x).any() and np.isnan(y).any()
    assert (g(d, "depth") < 1e-2).any() and (g(d, "targets_3d")[:, 2] == 100.0).any()
    q = g(d, "queries")
    assert (q[:, 1] < 0).any() and (q[:, 1] > float(g(d, "wd"))).any() and (q[:, 2] > float(g(d, "ht"))).any()
    # tracks 5 / 6: exactly MIN_TRACK_LEN / one fewer visible frames; tracks 8 / 9 under the initialised rule alone: 4 / 3
    n, Sp, M = int(g(d, "n")), int(g(d, "Sp")), int(g(d, "M"))
    lo = n - Sp
    w = g(d, "weights")[:, 0].reshape(-1, Sp)
    vis_raw = g(d, "local_vis_out").reshape(-1, M, g(d, "local_vis_out").shape[1])
    mid = (vis_raw.shape[2] + 1) // 2 - 1
    count = lambda q: int(vis_raw[lo + 2 * (q // M), q % M, mid - 2 * (q // M):mid - 2 * (q // M) + Sp].sum())
    assert count(5) == 3 and count(6) == 2
    assert w[5].sum() == 3 and w[6].sum() == 0
    assert g(d, "patches_valid_out")[lo, 5] == 1 and g(d, "patches_valid_out")[lo, 6] == 0
    pv = g("d_init", "patches_valid_out")
    assert g("d_init", "patches_valid_in")[lo + 2, 0] == 0 and pv[lo + 2, 0] == 1 and pv[lo + 2, 1] == 0


@pytest.mark.parametrize("seed", range(40))
def test_threshold_equals_torch_quantile_bit_for_bit(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([1, 2, 3, 7, 64, 144, 1000, 4097, 28800]))
    q = float(rng.choice([0.0, 1.0, 0.5, 0.7, 0.3, rng.random(), rng.random()]))
    v = rng.random(n).astype(np.float32)
    if seed % 5 == 0 and n > 3:
        v[rng.integers(0, n, n // 2)] = v[0]                                    # ties
    v = torch.as_tensor(v)
    want = torch.quantile(v, q)
    got = ou.quantile_threshold(v, q)
    assert ou.same_bits(got.numpy(), want.numpy()), (n, q, got.item(), want.item())
    v[n // 2] = float("nan")
    assert np.isnan(ou.quantile_threshold(v, q).item()) and np.isnan(torch.quantile(v, q).item())


def test_python_min_keeps_a_nan_quantile():
    assert np.isnan(min(float("nan"), 0.1)) and np.isnan(ou.static_threshold(torch.tensor([0.5, float("nan")]), 0.0, 0.1))


def test_library_and_op_are_declared():
    """The C entry point, the ctypes prototype, the torch op's schema and the source list (no GPU needed)."""
    from batrack_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "bt_observe_window") and hasattr(L, "bt_observe_workspace_bytes")
    assert "observe.hip" in _lib.SOURCES
    assert _lib.lib().bt_observe_workspace_bytes() >= 4
    s = str(_lib.torch_ops(strict=True).observe_window.default._schema)
    assert "Tensor(a!) patches_valid, Tensor(b!) patches_local" in s and "Tensor(g!) workspace" in s
    hdr = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "batrack_observe.h")).read()
    assert ctypes.sizeof(_lib.ObserveArgs) == 15 * 8 + 2 * 4 + 5 * 8 + 19 * 8 and "bt_observe_args" in hdr
