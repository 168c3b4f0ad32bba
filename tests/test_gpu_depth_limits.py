"""-m gpu: the depth metrics and the depth-map alignment (include/batrack_depth.h) at their limits, through the C ABI with raw
pointers so that pointer offsets, mask bytes and the workspace are the test's to choose.
  bt_depth_metrics      medians whose middle pair parts at a chosen key byte (gt and pred at different ones, odd and even counts,
                        as many invalid decoys as valid elements) against np.median exactly; the scalar path (gt / pred one float
                        past 16 bytes, a mask 1..3 bytes past 4) against the aligned call and numpy; mask bytes other than 0 / 1;
                        a dirty, reused and offset workspace; n = 0; the least-squares scaling on ever flatter preds against the
                        exact rational fit (1e-9, the gate of these metrics)
  bt_align_depth_maps   bit for bit against align_util.host_align_stats: constructed medians in both dtypes (every byte, the four
                        parities of c and the union count, ties, subnormals, c = 99 / 100 / 101); frames whose positive pixels
                        lie past the first grid-stride trip of every path, in place and out of place; a random sweep with ties,
                        zeros, negatives, infinities, NaN and skipped frames; NULL scales / overlap and a dirty workspace
Builders: depth_util.py, align_util.py (checked on the host by test_depth_limits_cpu.py)."""
import numpy as np
import pytest
import torch

from align_util import SECOND_TRIP, SWEEP_SEEDS, constructed_cases, host_align_stats, second_trip_scene, sweep_scene
from depth_util import (GT_LIMIT, LSTSQ_SWEEP, MEDIAN_NS, MEDIAN_PAIRS, check_gates, exact_lstsq_fit, fit_error, lstsq_sweep_case,
                        median_case, np_depth_metrics, valid_of)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALINGS = {"none": 0, "median": 1, "lstsq": 2}


def _lib():
    from batrack_amd import _lib as m
    return m, m.lib()


def carve(host, offset_bytes):
    """A device copy of `host` that starts offset_bytes past a 16-byte boundary (the allocator's blocks are 512-byte aligned).
    Returns (its address, the tensor that owns the memory, a view of the elements)."""
    host = np.array(host, copy=True)                                      # contiguous and writable, whatever came in
    raw = torch.zeros(host.nbytes + 64, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 16 == 0
    view = raw[offset_bytes:offset_bytes + host.nbytes]
    if host.nbytes:
        view.copy_(torch.from_numpy(host.view(np.uint8).reshape(-1)))
    return raw.data_ptr() + offset_bytes, raw, view


def workspace(nbytes, fill=None, offset=0):
    ws = torch.zeros(nbytes + offset, dtype=torch.uint8, device=DEV)
    if fill is not None:
        ws.fill_(fill)
    return ws, ws.data_ptr() + offset


def raw_metrics(gt, pred, mask, dmin, dmax, scaling, g_off=0, p_off=0, m_off=0, ws=None, ws_fill=None, ws_off=0):
    """bt_depth_metrics on device copies of the arrays; g_off / p_off in floats and m_off in bytes past a 16-byte boundary.
    `ws`: (tensor, address) to reuse; otherwise a new workspace, filled with ws_fill, starting ws_off bytes into its allocation."""
    m, L = _lib()
    n = gt.size
    gp, g_own, _ = carve(np.asarray(gt, np.float32), 4 * g_off)
    pp, p_own, _ = carve(np.asarray(pred, np.float32), 4 * p_off)
    mp, m_own = None, None
    if mask is not None:
        mp, m_own, _ = carve(np.asarray(mask, np.uint8), m_off)
    if ws is None:
        ws = workspace(int(L.bt_depth_metrics_workspace_bytes(n)), ws_fill, ws_off)
    out = torch.full((11,), -1.0, dtype=torch.float64, device=DEV)
    m.check(L.bt_depth_metrics(gp, pp, mp, n, float(dmin), float(dmax), SCALINGS[scaling], ws[1], out.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), "bt_depth_metrics")
    return out.cpu().numpy()


# ---------------------------------------------------------------------- bt_depth_metrics: constructed medians
PAIR = {p[0]: p for p in MEDIAN_PAIRS}
# (gt pair, pred pair): different divergence bytes in one call; gt pairs are finite, the pred median is never zero
MEDIAN_COMBOS = [("one_four", "next_b3"), ("across_sign", "next_b1"), ("next_b3", "one_four"), ("next_b2", "across_sign_2"),
                 ("next_b1", "subnormal_b3"), ("next_b0", "tied"), ("tied", "next_b2"), ("subnormal_b2", "huge_inf"),
                 ("subnormal_b3", "next_b0"), ("next_negative", "subnormal_b2"), ("tied", "tied")]


@pytest.mark.parametrize("gname,pname", MEDIAN_COMBOS)
def test_constructed_medians_are_numpy_medians_exactly(gname, pname):
    for n in MEDIAN_NS:
        gt, pred, mask = median_case(PAIR[gname][1:3], PAIR[pname][1:3], n, seed=n)
        v = valid_of(gt, mask, -GT_LIMIT, GT_LIMIT)
        with np.errstate(all="ignore"):
            want = np.median(gt[v].astype(np.float64)) / np.median(pred[v].astype(np.float64))
        for m_off in (0, 1):                                              # the vectorised and the scalar path
            r = raw_metrics(gt, pred, mask, -GT_LIMIT, GT_LIMIT, "median", m_off=m_off)
            assert r[8] == n == v.sum(), (n, r[8])
            assert r[9] == want, (gname, pname, n, m_off, r[9], want)


# ---------------------------------------------------------------------- bt_depth_metrics: the scalar path
def depth_case(n, seed=0):
    """Depths as the metrics see them: about a tenth masked out, some gt outside (0.5, 15); element 0 valid."""
    rng = np.random.default_rng(seed + n)
    gt = np.exp(rng.uniform(-1.0, 3.0, n)).astype(np.float32)
    pred = (gt * 0.4 * np.exp(0.3 * rng.standard_normal(n))).astype(np.float32)
    mask = (rng.random(n) < 0.9).astype(np.uint8)
    gt[0], mask[0] = 2.0, 1
    return gt, pred, mask


OFFSETS = [(1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3), (1, 1, 1), (1, 1, 2), (1, 1, 3)]


@pytest.mark.parametrize("scaling", ["none", "median", "lstsq"])
@pytest.mark.parametrize("n", [1, 5, 2049, 5003])
def test_scalar_path_matches_the_aligned_call_and_numpy(n, scaling):
    """gt / pred one float past a 16-byte boundary, the mask 1..3 bytes past a 4-byte one, separately and together.  The counts,
    the valid count and the median ratio are those of the aligned call exactly; the five sums associate differently and are held
    to numpy by check_gates.  With lstsq s and t come out of moments merged in another order too: they are held to the aligned
    call's at 1e-9 (the fixture's gate for them) and a1..a3 to within one element's share (check_gates' own lstsq gate)."""
    gt, pred, mask = depth_case(n)
    ref = np_depth_metrics(gt, pred, mask, 0.5, 15.0, scaling)
    gates = check_gates
    if n == 1 and scaling != "none":
        # one element scaled onto its gt (2.0): the five error sums are zero but for the rounding of p (g / p) or s p + t, a few
        # ulp of g at most, here as in numpy; a relative gate on them would compare two roundings of zero
        def gates(r, ref, count, scaling):
            assert r[8] == count == 1 and (r[5:8] == 1).all() and (ref[5:8] == 1).all()
            assert np.abs(r[:5]).max() <= 8 * np.finfo(np.float64).eps and np.abs(ref[:5]).max() <= 8 * np.finfo(np.float64).eps
    base = raw_metrics(gt, pred, mask, 0.5, 15.0, scaling)
    gates(base, ref, ref[8], scaling)
    for g_off, p_off, m_off in OFFSETS:
        r = raw_metrics(gt, pred, mask, 0.5, 15.0, scaling, g_off, p_off, m_off)
        gates(r, ref, ref[8], scaling)
        if scaling == "lstsq":
            assert r[8] == base[8]
            assert np.abs(r[5:8] - base[5:8]).max() <= 1.0 / base[8]
            np.testing.assert_allclose(r[9:11], base[9:11], rtol=1e-9)
        else:
            assert r[5:10].tobytes() == base[5:10].tobytes(), (g_off, p_off, m_off, r[5:10], base[5:10])
    if n == 5003:                                                         # no mask: the scalar path's `mask ? ... : true`
        r0, r1 = raw_metrics(gt, pred, None, 0.5, 15.0, scaling), raw_metrics(gt, pred, None, 0.5, 15.0, scaling, 1, 1)
        check_gates(r1, np_depth_metrics(gt, pred, None, 0.5, 15.0, scaling), r0[8], scaling)


@pytest.mark.parametrize("scaling", ["none", "median", "lstsq"])
def test_any_nonzero_mask_byte_is_true(scaling):
    gt, pred, mask = depth_case(5003, seed=1)
    rng = np.random.default_rng(5)
    loud = np.where(mask != 0, rng.choice(np.array([1, 2, 0x80, 0xFF], np.uint8), mask.size), 0).astype(np.uint8)
    assert set(np.unique(loud)) == {0, 1, 2, 0x80, 0xFF}
    for m_off in (0, 3):
        a = raw_metrics(gt, pred, mask, 0.5, 15.0, scaling, m_off=m_off)
        b = raw_metrics(gt, pred, loud, 0.5, 15.0, scaling, m_off=m_off)
        assert a.tobytes() == b.tobytes() and a[8] > 0


# ---------------------------------------------------------------------- bt_depth_metrics: the workspace, n = 0
@pytest.mark.parametrize("scaling", ["none", "median", "lstsq"])
def test_dirty_reused_and_offset_workspace(scaling):
    m, L = _lib()
    gt, pred, mask = depth_case(5003, seed=2)
    ws = workspace(int(L.bt_depth_metrics_workspace_bytes(gt.size)), 0xFF, offset=16)   # 16-byte aligned, no more
    assert ws[1] % 32 == 16
    first = raw_metrics(gt, pred, mask, 0.5, 15.0, scaling, ws=ws)
    second = raw_metrics(gt, pred, mask, 0.5, 15.0, scaling, ws=ws)       # on what the first call left
    fresh = raw_metrics(gt, pred, mask, 0.5, 15.0, scaling)
    assert first.tobytes() == second.tobytes() == fresh.tobytes()
    check_gates(first, np_depth_metrics(gt, pred, mask, 0.5, 15.0, scaling), first[8], scaling)


@pytest.mark.parametrize("scaling", ["none", "median", "lstsq"])
def test_no_elements_give_nan_metrics_and_a_count_of_zero(scaling):
    e = np.zeros(0, np.float32)
    for ws_fill in (None, 0xFF):
        r = raw_metrics(e, e, None, 0.5, 15.0, scaling, ws_fill=ws_fill)
        assert r[8] == 0 and np.isnan(r[:8]).all(), r


# ---------------------------------------------------------------------- bt_depth_metrics: least-squares conditioning
@pytest.mark.parametrize("index", range(len(LSTSQ_SWEEP)))
def test_lstsq_scaling_on_a_nearly_flat_pred(index, capsys):
    """pred = c + sigma randn down to a relative spread of 2.5e-7 and to two adjacent float32 values: np.linalg.lstsq calls every
    one full rank (test_depth_limits_cpu.py), so the kernel owes its answer.  The fit s p + t is held to the exact rational
    least-squares fit at 1e-9 relative to max |fit|, the gate of these metrics (numpy's SVD stays below 1e-15), and all eleven
    outputs to check_gates against numpy.
    Measured on the MI355X, fit error by sweep point (profiles/r13_depth_limits.txt): the raw normal equations this kernel first
    solved 1.7e-15, 1.3e-11, 3.6e-9, 2.3e-7, 2.6e-5, 5.1e-6, 8.7e-4, 7.0e-3; the centred moments 2.1e-16, 1.6e-16, 1.4e-16, 1.4e-16,
    2.8e-16, 1.8e-16, 5.3e-16, 3.7e-15 (the last is numpy's own figure: |s| is 42 there and s p + t cancels from 3400 to 161)."""
    pred, gt = lstsq_sweep_case(index)
    s_ref, t_ref, fit = exact_lstsq_fit(pred, gt)
    r = raw_metrics(gt, pred, None, 1e-2, 1e3, "lstsq")
    err = fit_error(r[9], r[10], pred, fit)
    with capsys.disabled():
        print(f"\n  lstsq sweep {LSTSQ_SWEEP[index]}: s {r[9]!r} (exact {s_ref!r}) t {r[10]!r} (exact {t_ref!r}) fit error {err:.2e}")
    assert err <= 1e-9, (LSTSQ_SWEEP[index], err)
    ref = np_depth_metrics(gt, pred, None, 1e-2, 1e3, "lstsq")
    assert ref[8] == pred.size
    check_gates(r, ref, ref[8], "lstsq")
    np.testing.assert_allclose(s_ref * pred.astype(np.float64) + t_ref, fit, rtol=1e-9)    # (the rounded s, t restate the fit)


# ---------------------------------------------------------------------- bt_align_depth_maps
def assert_same(out, ref, what=""):
    """Exactly equal: NaN at the same places, the bits of every other element equal."""
    assert out.dtype == ref.dtype and out.shape == ref.shape, what
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(out), nan), what
    u = f"u{ref.dtype.itemsize}"
    a, b = np.ascontiguousarray(out[~nan]).view(u), np.ascontiguousarray(ref[~nan]).view(u)
    assert np.array_equal(a, b), (what, np.flatnonzero(a != b)[:8])


SENTINEL = -7.0


def raw_align(maps, in_place=False, offset=0, want_scales=True, want_overlap=True, ws_fill=None):
    """bt_align_depth_maps on a device copy of maps [T, hw]; `offset` elements past a 16-byte boundary; out of place into a buffer
    prefilled with SENTINEL.  Returns aligned, scales, overlap (None where not asked for)."""
    m, L = _lib()
    T, hw = maps.shape
    dt = m.BT_DEPTH_F64 if maps.dtype == np.float64 else m.BT_DEPTH_F32
    src, s_own, s_view = carve(maps, offset * maps.dtype.itemsize)
    if in_place:
        dst, d_own, d_view = src, s_own, s_view
    else:
        dst, d_own, d_view = carve(np.full(maps.shape, SENTINEL, maps.dtype), offset * maps.dtype.itemsize)
    scales = torch.full((T,), 123.0, dtype=torch.float64, device=DEV) if want_scales else None
    overlap = torch.full((T,), -5, dtype=torch.int64, device=DEV) if want_overlap else None
    ws, wp = workspace(int(L.bt_align_depth_maps_workspace_bytes(hw, dt)), ws_fill)
    m.check(L.bt_align_depth_maps(src, dst, T, hw, dt, None if scales is None else scales.data_ptr(),
                                  None if overlap is None else overlap.data_ptr(), wp, torch.cuda.current_stream().cuda_stream),
            "bt_align_depth_maps")
    out = d_view.cpu().numpy().view(maps.dtype).reshape(T, hw)
    if not in_place:
        assert np.array_equal(s_view.cpu().numpy(), np.ascontiguousarray(maps).view(np.uint8).reshape(-1))   # the input is left alone
    return out, None if scales is None else scales.cpu().numpy(), None if overlap is None else overlap.cpu().numpy()


def check_align(maps, ref=None, what="", **kw):
    ref = host_align_stats(maps) if ref is None else ref
    out, scales, overlap = raw_align(maps, **kw)
    assert_same(out, ref[0], what)
    assert_same(scales, ref[1], what)
    assert np.array_equal(overlap, ref[2]), (what, overlap, ref[2])
    return out


@pytest.mark.parametrize("hw", [100, 101, 104])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constructed_alignment_medians(dtype, hw):
    for label, maps, c, union, _, _ in constructed_cases(dtype, hw):
        ref = host_align_stats(maps)
        assert ref[2][-1] == c and (c < 100 or ref[3][-1] == union), label
        check_align(maps, ref, label)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("dtype,hw,offset,per_thread", SECOND_TRIP)
def test_second_trip_of_the_grid_stride_loops(dtype, hw, offset, per_thread, in_place):
    """Frame 2 is positive only past the histogram pass's first trip: a pass that dropped its tail would see c < 100 and skip the
    frame; a write pass that dropped its tail would leave the sentinel (out of place) or the unscaled map (in place)."""
    maps, ref = second_trip_scene(dtype, hw, per_thread)
    assert ref[2][2] >= 100 and not np.isnan(ref[1][1:]).any()
    check_align(maps, ref, in_place=in_place, offset=offset)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_random_sweep_matches_the_host(seed, dtype):
    maps = sweep_scene(seed, dtype)
    check_align(maps, in_place=bool(seed & 1), offset=(seed >> 1) & 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_null_outputs_and_a_dirty_workspace(dtype):
    maps = sweep_scene(20, dtype)                                         # T = 9, hw = 513: skipped and scaled frames
    ref = host_align_stats(maps)
    assert np.isnan(ref[1][1:]).any() and not np.isnan(ref[1][1:]).all()
    first = check_align(maps, ref)
    for ws_fill, ws_sc, ws_ov in ((0xFF, True, True), (None, False, True), (None, True, False), (0xFF, False, False), (0xFF, True, True)):
        out, scales, overlap = raw_align(maps, want_scales=ws_sc, want_overlap=ws_ov, ws_fill=ws_fill)
        assert out.tobytes() == first.tobytes()
        if scales is not None:
            assert_same(scales, ref[1])
        if overlap is not None:
            assert np.array_equal(overlap, ref[2])
