"""CPU half of the depth kernels' limit tests (test_gpu_depth_limits.py): the builders and the sweeps cover what they claim.
  every constructed pair is the middle pair of its array and first differs at the stated byte of the kernel's key;
  the alignment scenes have the stated c, union count and middle pairs, and cover the four parities, the bytes and c = 99 .. 101;
  the random sweep holds skipped and scaled frames and both parities of c and of the union count;
  the second-trip shapes exceed what one trip of each kernel covers (the constants are read back from depth_align.hip);
  np.linalg.lstsq calls every point of the conditioning sweep full rank and is itself within 1e-15 of the exact rational fit
  (the two-valued pred: within what evaluating s p + t in float64 allows)."""
import os
import re

import numpy as np
import pytest

from align_util import (HIST_THREADS, SECOND_TRIP, SWEEP_HW, SWEEP_SEEDS, SWEEP_T, WRITE_THREADS, constructed_cases, host_align_stats,
                        positive_pair, sweep_scene)
from depth_util import (GT_LIMIT, LSTSQ_N, LSTSQ_SWEEP, MEDIAN_NS, MEDIAN_PAIRS, exact_lstsq_fit, f32_key, f32_unkey, first_diff_byte,
                        fit_error, lstsq_sweep_case, median_case, middle_pair, valid_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------- bt_depth_metrics
def test_the_host_key_orders_float32_as_the_kernel_does():
    x = np.array([-np.inf, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, np.inf], np.float32)
    k = f32_key(x)
    assert (np.diff(k.astype(np.int64)) >= 0).all() and k[4] == k[5] == 0x80000000
    back = f32_unkey(k)
    assert np.array_equal(back, x) and not np.signbit(back[4])           # -0 and +0 are one key, decoded as +0


def test_median_pairs_first_differ_at_the_stated_byte():
    bytes_seen = set()
    for name, lo, hi, b, finite in MEDIAN_PAIRS:
        assert lo <= hi and first_diff_byte(f32_key(lo)[0], f32_key(hi)[0], 4) == b, name
        assert finite == bool(np.isfinite(hi))
        bytes_seen.add(b)
    assert bytes_seen == {None, 0, 1, 2, 3}
    sub = [p for p in MEDIAN_PAIRS if p[0].startswith("subnormal")]
    assert sub and all(0 < p[1] < p[2] < np.finfo(np.float32).tiny for p in sub)
    nxt = [p for p in MEDIAN_PAIRS if p[0].startswith("next")]
    assert {p[3] for p in nxt} == {0, 1, 2, 3} and all(np.nextafter(p[1], np.float32(np.inf)) == p[2] for p in nxt)


@pytest.mark.parametrize("n", MEDIAN_NS)
def test_median_cases_have_the_pairs_in_the_middle_and_decoys_that_would_move_them(n):
    pair = {p[0]: p for p in MEDIAN_PAIRS}
    for gname, pname in (("one_four", "next_b3"), ("across_sign", "huge_inf"), ("subnormal_b2", "tied"), ("next_b1", "across_sign_2")):
        gt, pred, mask = median_case(pair[gname][1:3], pair[pname][1:3], n, seed=n)
        v = valid_of(gt, mask, -GT_LIMIT, GT_LIMIT)
        assert v.sum() == n and gt.size == 2 * n
        for x, (_, lo, hi, _, _) in ((gt, pair[gname]), (pred, pair[pname])):
            a, b = middle_pair(f32_key(x[v]))
            assert a == f32_key(lo)[0] and b == (f32_key(hi)[0] if n % 2 == 0 else f32_key(lo)[0])
            s = np.sort(x[v])
            assert n < 2 or s[(n - 1) // 2 + 1] == hi                      # an odd count has hi right above the median
            assert not np.isnan(x[v]).any()
        d = ~v
        assert ((mask[d] == 0) | ~((gt[d] > -GT_LIMIT) & (gt[d] < GT_LIMIT))).all()
        if n >= 63:
            assert (mask[d] == 0).any() and (mask[d] != 0).any() and np.isnan(gt[d]).any() and np.isnan(pred[d]).any()
            assert (gt[d] == GT_LIMIT).any() and (gt[d] == -GT_LIMIT).any()
            with np.errstate(all="ignore"):
                assert np.median(gt[mask != 0].astype(np.float64)) != np.median(gt[v].astype(np.float64)) or np.isnan(np.median(gt[mask != 0]))


# ---------------------------------------------------------------------- the least-squares sweep
@pytest.mark.parametrize("index", range(len(LSTSQ_SWEEP)))
def test_numpy_lstsq_is_full_rank_and_exact_on_the_sweep(index):
    pred, gt = lstsq_sweep_case(index)
    assert pred.size == LSTSQ_N and np.unique(pred).size >= 2
    p, g = pred.astype(np.float64), gt.astype(np.float64)
    (s, t), _, rank, sv = np.linalg.lstsq(np.stack([p, np.ones_like(p)], 1), g, rcond=None)
    s_ref, t_ref, fit = exact_lstsq_fit(pred, gt)
    assert rank == 2 and sv[1] / sv[0] > 100 * np.finfo(np.float64).eps * LSTSQ_N
    cap = 1e-15
    if LSTSQ_SWEEP[index][1] == "two values":
        # the noise over a spread of one float32 step makes |s| about 40, and s p + t cancels from 3400 down to 161: evaluating
        # it in float64 rounds s p, t and the sum by eps each, whoever supplies s and t
        assert np.unique(pred).size == 2 and abs((pred == 80).mean() - 0.5) < 0.1
        cap = 4 * np.finfo(np.float64).eps * (abs(s_ref) * p.max() + abs(t_ref)) / np.abs(fit).max()
        assert 1e-15 < cap < 1e-13
    assert fit_error(s, t, pred, fit) <= cap
    assert fit_error(s_ref, t_ref, pred, fit) <= cap                      # the rounded exact (s, t) restate the fit


# ---------------------------------------------------------------------- bt_align_depth_maps
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_positive_pairs_first_differ_at_the_stated_byte(dtype):
    nb = np.dtype(dtype).itemsize
    u = f"u{nb}"
    for b in range(nb):
        lo, hi = positive_pair(dtype, b)
        assert lo < hi and first_diff_byte(lo, hi, nb) == b
        v = np.array([lo, hi], u).view(dtype)
        assert (v > 0).all() and np.isfinite(v).all() and (v >= np.finfo(dtype).tiny).all()
    for b in range(nb // 2, nb):
        lo, hi = positive_pair(dtype, b, "subnormal")
        v = np.array([lo, hi], u).view(dtype)
        assert first_diff_byte(lo, hi, nb) == b and (v > 0).all() and (v < np.finfo(dtype).tiny).all()


@pytest.mark.parametrize("hw", [100, 101, 104])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constructed_alignment_scenes_cover_what_they_claim(dtype, hw):
    nb = np.dtype(dtype).itemsize
    u = f"u{nb}"
    seen, parities, cs = set(), set(), set()
    for label, maps, c, union, b, pb in constructed_cases(dtype, hw):
        T = maps.shape[0]
        out, scales, overlap, un = host_align_stats(maps)
        assert overlap[-1] == c, label
        cs.add(c)
        if T == 3:
            assert overlap[1] < 100 and np.array_equal(out[1].view(u), maps[1].view(u)), label   # frame 1 skipped: aligned[1] = maps[1]
        if c < 100:
            assert np.isnan(scales[-1])
            continue
        assert un[-1] == union and (T == 2 or union != 2 * c), label
        prev, cur = out[-2], maps[-1]
        m = (prev > 0) & (cur > 0)
        pv = prev[m] if T == 2 else np.concatenate((out[0][(out[0] > 0) & (prev > 0)], prev[m]))
        cl, cu = middle_pair(cur[m].view(u))
        pl, pu = middle_pair(pv.view(u))
        assert first_diff_byte(cl, cu, nb) == (b if c % 2 == 0 else None), label      # (an odd count selects one element twice)
        assert first_diff_byte(pl, pu, nb) == (pb if union % 2 == 0 else None), label
        if label.startswith("subnormal"):
            assert cur[m].view(u)[np.argsort(cur[m])][(c - 1) // 2] < np.array([np.finfo(dtype).tiny], dtype).view(u)[0]
        if T == 3 and not label.startswith(("tied", "subnormal", "threshold")):
            seen.add((b, pb))
            parities.add((b, c % 2, union % 2))
    assert {b for b, _ in seen} == set(range(nb)) and all(b != pb for b, pb in seen)
    want_c = {99, 100} | ({101} if hw >= 101 else set())
    assert cs == want_c
    if hw >= 101:
        assert parities == {(b, i, j) for b in range(nb) for i in (0, 1) for j in (0, 1)}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_random_sweep_skips_and_scales_at_every_parity(dtype):
    assert len(SWEEP_SEEDS) == 24 == len(SWEEP_T) * len(SWEEP_HW)
    shapes = set()
    by_T = {T: dict(skip=0, scale=0, c=set(), union=set(), both=0) for T in SWEEP_T}
    special = set()
    for seed in SWEEP_SEEDS:
        maps = sweep_scene(seed, dtype)
        T, hw = maps.shape
        shapes.add((T, hw))
        out, scales, overlap, union = host_align_stats(maps)
        g = by_T[T]
        skipped = overlap[1:] < 100
        g["skip"] += int(skipped.sum())
        g["scale"] += int((~skipped).sum())
        g["both"] += int(skipped.any() and (~skipped).any())
        g["c"] |= {int(c) % 2 for c in overlap[1:][~skipped]}
        g["union"] |= {int(n) % 2 for i, n in enumerate(union) if i >= 2 and overlap[i] >= 100}
        assert np.isfinite(scales[1:][~skipped]).all() and (scales[1:][~skipped] > 0).all()   # no chain dies of a NaN scale
        for name, hit in (("zero", (maps == 0) & ~np.signbit(maps)), ("-zero", (maps == 0) & np.signbit(maps)), ("neg", maps < 0),
                          ("inf", maps == np.inf), ("-inf", maps == -np.inf), ("nan", np.isnan(maps))):
            if hit.any():
                special.add(name)
        vals, counts = np.unique(maps[maps > 0], return_counts=True)
        assert counts.max() >= 3                                          # ties
    assert shapes == {(T, hw) for T in SWEEP_T for hw in SWEEP_HW}
    assert special == {"zero", "-zero", "neg", "inf", "-inf", "nan"}
    for T, g in by_T.items():
        assert g["skip"] > 0 and g["scale"] > 0 and g["c"] == {0, 1}, (T, g)
        if T >= 3:
            assert g["union"] == {0, 1} and g["both"] > 0, (T, g)       # skip and scale alternate along one chain


def test_second_trip_shapes_exceed_one_trip_of_each_kernel():
    src = open(os.path.join(ROOT, "batrack_amd", "csrc", "depth_align.hip")).read()
    # depth_align.hip:28-29
    assert re.search(r"constexpr int kHistThreads = 512, kHistBlocks = 256;", src)
    assert re.search(r"constexpr int kWriteThreads = 256, kWriteBlocks = 1024;", src)
    assert HIST_THREADS == 512 * 256 == 131_072 and WRITE_THREADS == 256 * 1024 == 262_144
    paths = set()
    for dtype, hw, offset, per_thread in SECOND_TRIP:
        nb = np.dtype(dtype).itemsize
        vec = offset == 0 and (hw * nb) % 16 == 0                        # depth_align.hip: run()'s choice of path
        assert per_thread == (16 // nb if vec else 1)
        assert hw > WRITE_THREADS * per_thread > HIST_THREADS * per_thread
        assert hw < 2 * HIST_THREADS * per_thread + WRITE_THREADS * per_thread   # no larger than it needs to be
        paths.add((nb, vec, offset))
    assert paths == {(4, True, 0), (8, True, 0), (4, False, 0), (8, False, 0), (4, False, 1)}
