"""bt_observe_window at its limits (include/batrack_observe.h, batrack_amd/csrc/observe.hip), the op against the torch
restatement tests/observe_util.window_observations_ref on the same GPU tensors, every output and every buffer bit for
bit: query counts around the workgroup's block of 32 tracks and the wave, windows of 1, 2 and 12 frames filled to 1,
S - 1 and S, no edges at all, every optional pointer NULL, quantile ranks that are integers and fractional, the
interpolated pair inside and across groups of tied scores, all scores equal, 28,800 scores (29 passes of the select's
workgroup), and every invalid argument of the header."""
import ctypes

import numpy as np
import pytest
import torch

import observe_util as ou
from batrack_amd import _lib
from batrack_amd.frontend.observe import ObserveConfig, window_observations

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def compare(args, kw, desc=""):
    a1, k1 = ou.clone_call(args, kw)
    a2, k2 = ou.clone_call(args, kw)
    got = ou.results(window_observations(*a1, **k1), k1)
    want = ou.results(ou.window_observations_ref(*a2, **k2), k2)
    for k in ou.OUTPUTS:
        if want[k] is None:
            assert got[k] is None, k
        else:
            assert ou.same_bits(got[k], want[k]), f"{desc}: {k} differs from the restatement"
    return got


def split(Nq, Sp):
    """(M, kf_stride) with Nq = ceil(Sp / kf_stride) * M, the most keyframes that divide Nq."""
    for Q in range(min(Sp, 6), 0, -1):
        for kf in range(1, Sp + 1):
            if -(-Sp // kf) == Q and Nq % Q == 0:
                return Nq // Q, kf
    raise AssertionError


@pytest.mark.parametrize("S,Sp", [(1, 1), (2, 1), (2, 2), (12, 1), (12, 11), (12, 12)])
@pytest.mark.parametrize("Nq", [1, 63, 64, 65, 200])
def test_shapes(Nq, S, Sp):
    M, kf = split(Nq, Sp)
    init = (Nq + S) % 2 == 0
    cfg = ObserveConfig(STATIC_QUANTILE=0.3 if Sp == S else 0.0, MIN_TRACK_LEN=3 if S > 2 else 1)
    args, kw = ou.random_inputs(100 * Nq + 10 * S + Sp, Nq, M, S, Sp, kf, DEV, cfg=cfg, init=init, n=Sp + (2 if Sp > 1 else 0))
    compare(args, kw, f"Nq {Nq} M {M} S {S} S' {Sp} kf {kf}")


@pytest.mark.parametrize("q", [0.0, 1.0, 0.5, 0.3, 0.123])
def test_quantile_ranks(q):
    """q = 0 and 1 (and 0.5 of an odd count) are integer ranks, the others interpolate; the scores lie below
    STATIC_THRESHOLD so that the quantile is the threshold."""
    S, Nq, M, kf = 5, 21, 7, 2                                          # 105 scores: rank 52 at q = 0.5
    dyn = np.random.default_rng(5).uniform(0.92, 1.0, (S, Nq))
    args, kw = ou.random_inputs(7, Nq, M, S, S, kf, DEV, cfg=ObserveConfig(STATIC_QUANTILE=q), dyn=dyn)
    got = compare(args, kw, f"q {q}")
    if q == 0.5:
        assert got["weights_pose"].any() and not np.array_equal(got["weights_pose"], got["weights"])


@pytest.mark.parametrize("q", [0.07, 0.36, 0.5, 1.0])
def test_quantile_pair_against_tie_groups(q):
    """Eight scores in three tie groups of 3, 2 and 3: counted from the largest static score the interpolated pair is ranks
    (0, 1) inside the first group, (2, 3) across two groups, (3, 4) inside the middle group, and the last element alone."""
    S, Nq = 2, 4
    M, kf = split(Nq, S)
    dyn = np.array([[0.99, 0.95, 0.97, 0.99], [0.95, 0.99, 0.95, 0.97]])
    cfg = ObserveConfig(STATIC_QUANTILE=q)
    args, kw = ou.random_inputs(21, Nq, M, S, S, kf, DEV, cfg=cfg, dyn=dyn)
    th = ou.static_threshold(args[3].cpu(), cfg.STATIC_QUANTILE, cfg.STATIC_THRESHOLD)
    assert np.isfinite(th) and th < cfg.STATIC_THRESHOLD
    compare(args, kw, f"tie groups, q {q}")


@pytest.mark.parametrize("value,any_static", [(0.95, True), (0.5, True), (float("nan"), False)])
def test_all_scores_equal(value, any_static):
    S, Nq, M, kf = 4, 40, 20, 2
    args, kw = ou.random_inputs(8, Nq, M, S, S, kf, DEV, cfg=ObserveConfig(STATIC_QUANTILE=0.4), dyn=np.full((S, Nq), value))
    got = compare(args, kw, f"all dyn = {value}")
    assert bool(got["weights_pose"].any()) == any_static
    if any_static:
        assert np.array_equal(got["weights_pose"], got["weights"])


@pytest.mark.parametrize("q", [0.0, 0.37])
def test_28800_scores(q):
    """The DAVIS shape: 12 x 2,400 scores, 29 passes of the select's 1,024 lanes; ties among them."""
    S, Nq, M, kf = 12, 2400, 400, 2
    rng = np.random.default_rng(9)
    dyn = rng.uniform(0.9, 1.0, (S, Nq)).astype(np.float32)
    dyn[rng.random((S, Nq)) < 0.2] = dyn[3, 3]
    args, kw = ou.random_inputs(9, Nq, M, S, S, kf, DEV, H=60, W=80, cfg=ObserveConfig(STATIC_QUANTILE=q), dyn=dyn)
    compare(args, kw, f"28,800 scores, q {q}")


def test_null_optional_buffers_and_no_tail():
    S, Nq, M, kf = 6, 66, 22, 2
    args, kw = ou.random_inputs(11, Nq, M, S, S, kf, DEV, cfg=ObserveConfig(VIS_THRESHOLD=None))
    for drop in (("local_monodisp",), ("local_vis", "local_static"), ("local_weights",), ou.BUFFERS[1:]):
        compare(args, dict(kw, **{k: None for k in drop}), f"without {drop}")
    a = list(args)
    a[5] = None                                                          # no depth maps: no query sampling
    assert compare(a, kw, "no dmaps")["query_disp"] is None
    args, kw = ou.random_inputs(12, Nq, M, S, S, kf, DEV, interp_shape=None, S_local=5)
    compare(args, kw, "no tail, short window buffer")


def test_far_query_coordinates():
    """The query depth at finite coordinates beyond int32 (bilinear_clamped of csrc/sample_taps.hpp): the reference's floor
    becomes INT_MIN on either side, the clamped indices coincide, the weights are of the coordinate's size and cancel: d is 0
    or a rounding residue (query_disp = 100 where it is 0), and NaN where the product of two far weights overflows."""
    S, Nq, M, kf = 6, 66, 22, 2
    args, kw = ou.random_inputs(14, Nq, M, S, S, kf, DEV, interp_shape=None)
    far = [(3e9, 5.0), (-3e9, 5.5), (7.25, 3e9), (7.25, 2.0 ** 31), (2.0 ** 31, 9.0), (1e30, 4.5), (5.5, -1e30), (5e37, 7.0),
           (3e9, -1e30), (1e30, 3e9), (2.0 ** 24 + 2, 6.5), (-(2.0 ** 24 + 2), 2.0 ** 24 + 2)]
    args[4][0, 10:10 + len(far), 1:] = torch.tensor(far, device=DEV)
    got = compare(args, kw, "far queries")["query_disp"][10:10 + len(far)]
    assert got[0] == 100.0 and got[4] == 100.0 and np.isnan(got[8]) and np.isnan(got[9]) and np.isfinite(got[[0, 1, 2, 3, 4, 5, 6, 7, 10, 11]]).all()


# ---- the C ABI itself
def c_args(args, kw, outs):
    traj, depth, vis, dyn, queries, dmaps, ii, jj, kk = args
    S, Nq = traj.shape[1], traj.shape[2]
    N, M = kw["patches_valid"].shape
    cfg = kw["cfg"] or ObserveConfig()
    p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    ih, iw = kw["interp_shape"] or (0, 0)
    return _lib.ObserveArgs(S=S, Sp=kw["window"], Nq=Nq, E=Nq * kw["window"], n=kw["n"], M=M, N=N, kf_stride=kw["kf_stride"],
                            S_local=kw["patches_local"].shape[1], H=kw["image_size"][0], W=kw["image_size"][1], interp_w=iw, interp_h=ih,
                            padding=kw["padding"], min_track_len=cfg.MIN_TRACK_LEN, has_vis_threshold=int(cfg.VIS_THRESHOLD is not None),
                            is_initialized=int(kw["is_initialized"]), wd=kw["wd"], ht=kw["ht"], vis_threshold=cfg.VIS_THRESHOLD or 0.0,
                            static_quantile=cfg.STATIC_QUANTILE, static_threshold=cfg.STATIC_THRESHOLD, traj=p(traj), depth=p(depth),
                            vis=p(vis), dyn=p(dyn), queries=p(queries), dmaps=p(dmaps), ii=p(ii), jj=p(jj), kk=p(kk),
                            patches_valid=p(kw["patches_valid"]), patches_local=p(kw["patches_local"]), local_monodisp=p(kw["local_monodisp"]),
                            local_vis=p(kw["local_vis"]), local_static=p(kw["local_static"]), local_weights=p(kw["local_weights"]),
                            targets_3d=p(outs[0]), weights=p(outs[1]), weights_pose=p(outs[2]), query_disp=p(outs[3]))


def c_setup(seed=13, Nq=48, M=16, S=6, Sp=6, kf=2):
    args, kw = ou.random_inputs(seed, Nq, M, S, Sp, kf, DEV)
    E = Nq * Sp
    outs = [torch.full((max(E, 1), 3), -77.0, device=DEV), torch.full((max(E, 1), 2), -77.0, device=DEV),
            torch.full((max(E, 1), 2), -77.0, device=DEV), torch.full((max(Nq, 1),), -77.0, device=DEV)]
    ws = torch.zeros(16, device=DEV)
    return args, kw, outs, ws


def snapshot(kw, outs):
    return [t.clone() for t in list(outs) + [kw[k] for k in ("patches_valid",) + ou.BUFFERS]]


def unchanged(kw, outs, snap):
    return all(torch.equal(a, b) for a, b in zip(list(outs) + [kw[k] for k in ("patches_valid",) + ou.BUFFERS], snap))


def test_c_abi_equals_the_wrapper():
    args, kw, outs, ws = c_setup()
    a2, k2 = ou.clone_call(args, kw)
    a = c_args(args, kw, outs)
    assert _lib.lib().bt_observe_window(ctypes.byref(a), ws.data_ptr(), None) == _lib.BT_OK
    torch.cuda.synchronize()
    want = ou.results(window_observations(*a2, **k2), k2)
    got = ou.results((outs[0][None], outs[1][None], outs[2][None], outs[3]), kw)
    for k in ou.OUTPUTS:
        assert ou.same_bits(got[k], want[k]), k


def test_no_edges():
    """E = 0 (an empty window): BT_OK, nothing touched, through the C ABI and through the wrapper."""
    args, kw, outs, ws = c_setup(Nq=0, M=16, Sp=0)
    snap = snapshot(kw, outs)
    a = c_args(args, kw, outs)
    assert _lib.lib().bt_observe_window(ctypes.byref(a), ws.data_ptr(), None) == _lib.BT_OK
    torch.cuda.synchronize()
    assert unchanged(kw, outs, snap)
    t3, w, wp, qd = window_observations(*args, **kw)
    assert t3.shape == (1, 0, 3) and w.shape == (1, 0, 2) and wp.shape == (1, 0, 2) and qd.numel() == 0
    assert unchanged(kw, outs, snap)


INVALID = [(dict(S=0), "EINVAL"), (dict(Sp=-1), "EINVAL"), (dict(Sp=7), "EINVAL"), (dict(Nq=-1), "EINVAL"), (dict(M=0), "EINVAL"),
           (dict(Nq=47), "EINVAL"), (dict(E=287), "EINVAL"), (dict(kf_stride=0), "EINVAL"), (dict(kf_stride=3), "EINVAL"),
           (dict(N=0), "EINVAL"), (dict(n=5), "EINVAL"), (dict(n=12), "EINVAL"), (dict(S_local=0), "EINVAL"), (dict(H=0), "EINVAL"),
           (dict(W=0), "EINVAL"), (dict(interp_w=-1), "EINVAL"), (dict(interp_h=0), "EINVAL"), (dict(interp_w=0), "EINVAL"),
           (dict(padding=-1), "EINVAL"), (dict(static_quantile=-0.1), "EINVAL"), (dict(static_quantile=1.5), "EINVAL"),
           (dict(static_quantile=float("nan")), "EINVAL")] + \
          [({k: None}, "EINVAL") for k in ("traj", "depth", "vis", "dyn", "queries", "ii", "jj", "kk", "patches_valid", "patches_local",
                                          "targets_3d", "weights", "weights_pose", "query_disp")] + \
          [(dict(S=65, Sp=6), "EUNSUPPORTED"), (dict(S=1 << 19, Sp=6), "EUNSUPPORTED"), (dict(S_local=1 << 31), "EUNSUPPORTED"),
           (dict(N=1 << 28, n=9), "EUNSUPPORTED"), (dict(H=1 << 16, W=1 << 15), "EUNSUPPORTED")]


@pytest.fixture(scope="module")
def valid_call():
    return c_setup()


@pytest.mark.parametrize("change,status", INVALID, ids=[f"{next(iter(c))}={next(iter(c.values()))}" for c, _ in INVALID])
def test_invalid_arguments(valid_call, change, status):
    """Every refusal of the header returns its status before anything is enqueued: outputs and buffers keep their bytes."""
    args, kw, outs, ws = valid_call
    snap = snapshot(kw, outs)
    a = c_args(args, kw, outs)
    for k, v in change.items():
        setattr(a, k, v)
    assert _lib.lib().bt_observe_window(ctypes.byref(a), ws.data_ptr(), None) == getattr(_lib, "BT_" + status)
    torch.cuda.synchronize()
    assert unchanged(kw, outs, snap)


def test_null_struct_and_workspace(valid_call):
    args, kw, outs, ws = valid_call
    snap = snapshot(kw, outs)
    a = c_args(args, kw, outs)
    L = _lib.lib()
    assert L.bt_observe_window(None, ws.data_ptr(), None) == _lib.BT_EINVAL
    assert L.bt_observe_window(ctypes.byref(a), None, None) == _lib.BT_EINVAL
    torch.cuda.synchronize()
    assert unchanged(kw, outs, snap)
    assert L.bt_observe_workspace_bytes() <= ws.numel() * 4
