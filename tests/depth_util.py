"""A numpy restatement of the reference's depth metrics (main/global_refine/model/utils.py:187-265) as the kernels define
them (include/batrack_depth.h): float32 values, every per-element operation in float64, the limits compared and clamped as
float32 numbers.  Returns the 11 numbers of bt_depth_metrics.

Also what the limit tests of the depth kernels share (test_gpu_depth_limits.py, test_depth_limits_cpu.py): the kernels'
order-preserving float32 key on the host, arrays whose two middle elements are a chosen pair, the conditioning sweep of the
least-squares scaling and its exact rational fit."""
from fractions import Fraction

import numpy as np


def np_depth_metrics(gt, pred, mask=None, depth_min=1e-2, depth_max=1e2, scaling="median"):
    g = np.asarray(gt, np.float32).astype(np.float64).ravel()
    p = np.asarray(pred, np.float32).astype(np.float64).ravel()
    lo, hi = float(np.float32(depth_min)), float(np.float32(depth_max))
    valid = (g > lo) & (g < hi) & (np.ones(g.shape, bool) if mask is None else np.asarray(mask, bool).ravel())
    g, p = g[valid], p[valid]
    s, t = 1.0, 0.0
    with np.errstate(all="ignore"):
        if scaling == "median":
            s = np.median(g) / np.median(p) if g.size else np.nan
            p = p * s
        elif scaling == "lstsq" and g.size:
            s, t = np.linalg.lstsq(np.stack([p, np.ones_like(p)], 1), g, rcond=None)[0]
            p = s * p + t
        p[p < lo] = lo
        p[p > hi] = hi
        th = np.maximum(g / p, p / g)
        e = g - p
        m = [np.mean(np.abs(e) / g), np.mean(e ** 2 / g), np.mean(np.abs(np.log10(p) - np.log10(g))), np.sqrt(np.mean(e ** 2)),
             np.sqrt(np.mean((np.log(g) - np.log(p)) ** 2)), (th < 1.25).mean(), (th < 1.25 ** 2).mean(), (th < 1.25 ** 3).mean()]
    return np.array([float(x) for x in m] + [float(g.size), float(s), float(t)])


def check_gates(r, ref, count, scaling):
    """The suite's gates on bt_depth_metrics: the count exactly, the five sums 1e-9 relative, a1..a3 exactly (lstsq: within one
    element's share, SVD and the kernel round s and t differently)."""
    assert r[8] == count
    np.testing.assert_allclose(r[:5], ref[:5], rtol=1e-9)
    tol = 1.0 / count if scaling == "lstsq" else 0.0
    assert np.abs(r[5:8] - ref[5:8]).max() <= tol, (r[5:8], ref[5:8])


# ---------------------------------------------------------------------- keys and constructed medians
def f32_key(x):
    """radix_select.hpp's fkey on the host: uint32 keys that order float32 values as `<` does; -0 and +0 are one key."""
    u = np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def f32_unkey(k):
    k = np.atleast_1d(np.asarray(k)).astype(np.uint32)
    return np.where(k & 0x80000000, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def first_diff_byte(a, b, nbytes):
    """The first byte (0 = most significant) at which the integer keys a and b of nbytes bytes differ; None when equal."""
    x = int(a) ^ int(b)
    return None if x == 0 else nbytes - 1 - (x.bit_length() - 1) // 8


def middle_pair_keys(lo, hi, n, kmin, kmax, rng):
    """n integer keys (uint64) in [kmin, kmax], shuffled, whose sorted elements (n - 1) // 2 and the one after it are lo and hi:
    an even n has (lo, hi) as its middle pair, an odd n has lo alone in the middle and hi right above it.  Half of the other keys
    lie within 2^0, 2^8, 2^16 or 2^24 of the pair (they share its leading bytes, ties included), half anywhere in the range."""
    lo, hi, kmin, kmax = (np.uint64(int(v)) for v in (lo, hi, kmin, kmax))
    assert kmin <= lo <= hi <= kmax and n >= 1
    below = (n - 1) // 2
    above = n - below - min(n, 2)

    def fill(count, a, b, anchor, sign):
        far = rng.integers(a, b, count, dtype=np.uint64, endpoint=True)
        span = np.uint64(1) << rng.choice(np.array([0, 8, 16, 24], np.uint64), count)
        off = rng.integers(0, 1 << 24, count, dtype=np.uint64) % span
        near = np.where(off > anchor - a, a, anchor - off) if sign < 0 else np.where(off > b - anchor, b, anchor + off)
        return np.where(rng.random(count) < 0.5, near, far).astype(np.uint64)

    keys = np.concatenate([fill(below, kmin, lo, lo, -1), np.array([lo, hi][:min(n, 2)], np.uint64), fill(above, hi, kmax, hi, +1)])
    return rng.permutation(keys)


def middle_pair(keys):
    """(lower, upper) middle element of the sorted keys: the two selections the kernels make (equal for an odd count)."""
    s = np.sort(np.asarray(keys))
    return s[(s.size - 1) // 2], s[s.size // 2]


# (name, lo, hi, the key byte at which they first differ) as float32 bit patterns; `gt` says whether both can be a valid gt (finite)
_b = lambda u: np.array([u], np.uint32).view(np.float32)[0]
MEDIAN_PAIRS = [
    ("one_four", np.float32(1.0), np.float32(4.0), 0, True),
    ("across_sign", np.float32(-1.0), np.float32(1.0), 0, True),
    ("across_sign_2", np.float32(-1.0), np.float32(2.0), 0, True),       # for pred: a median that is not zero at even n
    ("next_b0", _b(0x3FFFFFFF), _b(0x40000000), 0, True),                # x and nextafter(x): the carry runs up to byte 0,
    ("next_b1", _b(0x3F80FFFF), _b(0x3F810000), 1, True),                # to byte 1,
    ("next_b2", _b(0x3F8000FF), _b(0x3F800100), 2, True),                # to byte 2,
    ("next_b3", np.float32(1.5), np.nextafter(np.float32(1.5), np.float32(2.0)), 3, True),   # nowhere
    ("next_negative", np.nextafter(np.float32(-2.5), np.float32(-3.0)), np.float32(-2.5), 3, True),
    ("tied", np.float32(0.75), np.float32(0.75), None, True),
    ("subnormal_b2", _b(0x00000003), _b(0x00000103), 2, True),
    ("subnormal_b3", _b(0x00000001), _b(0x00000002), 3, True),
    ("huge_inf", np.float32(3e38), np.float32(np.inf), 1, False),
]
MEDIAN_NS = (1, 2, 3, 4, 5, 63, 64, 65, 2047, 2048, 2049, 5003)
GT_LIMIT = np.float32(3.3e38)                                             # depth_min = -GT_LIMIT, depth_max = GT_LIMIT
_FILL = np.float32(3.2e38)                                                # the other valid values stay inside (-_FILL, _FILL)


def median_values(lo, hi, n, rng, allow_inf=False):
    """float32 [n] whose two middle elements are (lo, hi) (middle_pair_keys on the kernel's key); finite unless allow_inf."""
    kmin, kmax = int(f32_key(-_FILL)[0]), int(f32_key(np.float32(np.inf) if allow_inf else _FILL)[0])
    keys = middle_pair_keys(int(f32_key(lo)[0]), int(f32_key(hi)[0]), n, kmin, kmax, rng)
    return f32_unkey(keys)


def median_case(gt_pair, pred_pair, n, seed):
    """gt, pred (float32 [2n]) and mask (uint8 [2n]) for depth limits (-GT_LIMIT, GT_LIMIT): n valid elements whose gt and pred
    have the chosen middle pairs, and n decoys that are not valid — mask false, gt at or outside a limit, NaN gt — with extreme gt
    and pred values (NaN pred included) that would move a median if they were counted.  Shuffled."""
    rng = np.random.default_rng(seed)
    gv = median_values(gt_pair[0], gt_pair[1], n, rng)
    pv = median_values(pred_pair[0], pred_pair[1], n, rng, allow_inf=True)
    extreme = np.array([3.2e38, -3.2e38, 1e-45, -1e-45, 0.0, 65504.0, np.inf, -np.inf, np.nan], np.float32)
    outside = np.array([GT_LIMIT, -GT_LIMIT, np.inf, -np.inf, np.nan, np.float32(3.4e38), np.float32(-3.4e38)], np.float32)
    kind = rng.integers(0, 2, n)                                          # 0: mask false, any gt;  1: mask true, gt not inside
    gd = np.where(kind == 0, rng.choice(extreme, n), rng.choice(outside, n)).astype(np.float32)
    pd = rng.choice(extreme, n).astype(np.float32)
    md = np.where(kind == 0, 0, rng.choice(np.array([1, 2, 0x80, 0xFF], np.uint8), n)).astype(np.uint8)
    perm = rng.permutation(2 * n)
    gt, pred = np.concatenate([gv, gd])[perm], np.concatenate([pv, pd])[perm]
    mask = np.concatenate([np.ones(n, np.uint8), md])[perm]
    return gt, pred, mask


def valid_of(gt, mask, dmin, dmax):
    return (np.asarray(mask) != 0) & (gt > np.float32(dmin)) & (gt < np.float32(dmax))


# ---------------------------------------------------------------------- the least-squares conditioning sweep
LSTSQ_N = 1001
LSTSQ_SWEEP = [(5, 1.0), (5, 1e-2), (50, 1e-2), (50, 1e-3), (50, 1e-4), (80, 1e-4), (80, 2e-5), (80, "two values")]


def _lstsq_sweep():
    rng = np.random.default_rng(0)                                        # one stream through the points, in order
    cases = []
    for c, sigma in LSTSQ_SWEEP:
        if sigma == "two values":
            p = np.where(rng.random(LSTSQ_N) < 0.5, np.float32(c), np.nextafter(np.float32(c), np.float32(np.inf))).astype(np.float32)
        else:
            p = (c + sigma * rng.standard_normal(LSTSQ_N)).astype(np.float32)
        g = (2.0 * p.astype(np.float64) + 1.0 + 0.01 * rng.standard_normal(LSTSQ_N)).astype(np.float32)
        cases.append((p, g))
    return cases


_LSTSQ_CASES = []


def lstsq_sweep_case(index):
    """(pred, gt) float32 [LSTSQ_N] of sweep point `index`: pred = c + sigma randn (or 80 and nextafter(80), about half each),
    gt = 2 pred + 1 + 0.01 randn: ever flatter preds, all of which np.linalg.lstsq calls full rank."""
    if not _LSTSQ_CASES:
        _LSTSQ_CASES.extend(_lstsq_sweep())
    p, g = _LSTSQ_CASES[index]
    return p.copy(), g.copy()


def exact_lstsq_fit(pred, gt):
    """The least-squares fit of gt by [pred, 1] in exact rational arithmetic on the float32 values: (s, t, fit), the fitted values
    s p + t formed exactly and each rounded once to float64."""
    P, G = [Fraction(float(x)) for x in pred], [Fraction(float(x)) for x in gt]
    n = len(P)
    sp, sg = sum(P), sum(G)
    cpp = sum((n * x - sp) ** 2 for x in P)                               # n^2 sum (p - mean p)^2
    cpg = sum((n * x - sp) * (n * y - sg) for x, y in zip(P, G))
    assert cpp > 0
    s = cpg / cpp
    t = (sg - s * sp) / n
    return float(s), float(t), np.array([float(s * x + t) for x in P])


def fit_error(s, t, pred, fit):
    """max |s p + t - fit| / max |fit| in float64: what the 1e-9 of the metrics is asked of."""
    return float(np.abs(s * np.asarray(pred, np.float64) + t - fit).max() / np.abs(fit).max())
