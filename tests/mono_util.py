"""The mono-depth alignment (main/mono_depth/get_mono_depth.py:52-140) restated in numpy from its formulas, with the
intermediates bt_mono_align reports (include/batrack_depth.h): per-frame scales s and shifts c, the aligns (a_s, a_c, n) and
k.  Everything runs in the metric depth's dtype D as numpy's promotion rules (NEP 50) put it: the Python scalars of the
formulas take D, a float32 disparity widens where it meets a float64 value."""
import numpy as np


def restate(mono, metric):
    d = np.asarray(mono).astype(np.float32)
    m = np.asarray(metric)
    D = m.dtype.type
    T = m.shape[0]
    s, c = np.empty(T, D), np.empty(T, D)
    with np.errstate(all="ignore"):
        for t in range(T):
            g = D(1) / (m[t] + D(1e-8))
            g[(m[t] < D(2)) & (d[t] < np.float32(0.02))] = D(0.01)
            num = g - np.median(g) + D(1e-8)                                # D
            den = d[t] - np.median(d[t]) + np.float32(1e-8)                 # float32
            s[t] = np.median(num / den)
            c[t] = np.median(g - s[t] * d[t])
        p = s * c
        k = int(np.argmin(np.abs(p - np.median(p))))
        y = s[k] * d + c[k]                                                 # D (a numpy scalar is strong)
        n = np.percentile(y, 98) / D(2)
        depth = np.clip(D(1) / ((D(1) / n) * y), D(1e-4), D(1e4))
        depth[depth < D(1e-2)] = D(0)
    return depth, s, c, np.array([s[k], c[k], n], D), k


def percentile_gamma(n_elems, dtype):
    """numpy's gamma for the 98th percentile of n_elems values of `dtype` (method 'linear'): the fractional part of (n - 1) q."""
    q = np.true_divide(98, dtype(100))
    v = (n_elems - 1) * np.asanyarray(q)
    return float(v - np.floor(v))


def restate_frames(mono, metric):
    """restate with the per-frame medians taken along an axis of [T, hw] arrays: the same formulas in the same dtype, no loop
    over the frames in Python (restate is the authority; test_mono_limits_cpu.py holds this one to it bit for bit)."""
    d = np.asarray(mono).astype(np.float32)
    m = np.asarray(metric)
    D = m.dtype.type
    T = m.shape[0]
    d2, m2 = d.reshape(T, -1), m.reshape(T, -1)
    with np.errstate(all="ignore"):
        g = D(1) / (m2 + D(1e-8))
        g[(m2 < D(2)) & (d2 < np.float32(0.02))] = D(0.01)
        num = g - np.median(g, axis=1, keepdims=True) + D(1e-8)             # D
        den = d2 - np.median(d2, axis=1, keepdims=True) + np.float32(1e-8)  # float32
        s = np.median(num / den, axis=1)
        c = np.median(g - s[:, None] * d2, axis=1)
        p = s * c
        k = int(np.argmin(np.abs(p - np.median(p))))
        y = s[k] * d + c[k]
        n = np.percentile(y, 98) / D(2)
        depth = np.clip(D(1) / ((D(1) / n) * y), D(1e-4), D(1e4))
        depth[depth < D(1e-2)] = D(0)
    return depth, s, c, np.array([s[k], c[k], n], D), k


# ---------------------------------------------------------------------- keys and middle pairs (csrc/radix_select.hpp)
TIE = "tie"


def fkey(x):
    """The order-preserving key of float32 / float64 values as radix_select.hpp forms it (-0 and +0 are one key)."""
    x = np.ascontiguousarray(x)
    u = x.view(f"u{x.dtype.itemsize}")
    sign = u.dtype.type(1 << (8 * x.dtype.itemsize - 1))
    u = np.where(u == sign, u.dtype.type(0), u)
    return np.where(u & sign, ~u, u | sign)


def parting_byte(lo, hi):
    """The first byte (0: most significant) at which the keys of two values of one dtype differ; TIE if they are one key."""
    lo, hi = np.asarray(lo), np.asarray(hi)
    assert lo.dtype == hi.dtype
    x = int(fkey(lo).ravel()[0]) ^ int(fkey(hi).ravel()[0])
    return TIE if x == 0 else lo.dtype.itemsize - 1 - (x.bit_length() - 1) // 8


def middle_pair(x):
    """The two middle elements of a set without NaN (one element twice when the count is odd)."""
    v = np.sort(np.asarray(x).ravel())
    return v[(v.size - 1) // 2], v[v.size // 2]


def frame_values(d, m):
    """The four sets a frame's medians are taken over, by restate's formulas: g, d (in D, as the kernel keys it), the ratio and
    g - s d, with s the median of the ratio."""
    d, m = np.asarray(d, np.float32).ravel(), np.asarray(m).ravel()
    D = m.dtype.type
    with np.errstate(all="ignore"):
        g = D(1) / (m + D(1e-8))
        g[(m < D(2)) & (d < np.float32(0.02))] = D(0.01)
        ratio = (g - np.median(g) + D(1e-8)) / (d - np.median(d) + np.float32(1e-8))
        s = np.median(ratio)
        resid = g - s * d
    return {"g": g, "d": d.astype(D), "ratio": ratio.astype(D), "resid": resid}


SELECTIONS = ("g", "d", "ratio", "resid")


def frame_partings(d, m):
    """Per selection, the key byte at which the frame's middle pair parts (TIE: one key; None: the set holds a NaN)."""
    out = {}
    for name, v in frame_values(d, m).items():
        out[name] = None if np.isnan(v).any() else parting_byte(*middle_pair(v))
    return out


# ---------------------------------------------------------------------- constructed medians
def _around(lo, hi, below, above, hw, rng):
    """A frame's worth of one selection: lo and hi as the middle pair of hw values, the rest drawn from `below` / `above`."""
    nb = (hw - 1) // 2
    v = np.concatenate([below[:nb], [lo, hi], above[:hw - nb - 2]])
    assert v.size == hw and (below[:nb] < lo).all() and (above[:hw - nb - 2] > hi).all()
    return v[rng.permutation(hw)]


def _g_of(m):
    with np.errstate(all="ignore"):
        return m.dtype.type(1) / (m + m.dtype.type(1e-8))


def g_frame(dtype, hw, target, seed=0):
    """A frame whose g = 1 / (m + 1e-8) has a middle pair that parts at key byte `target` (TIE: one value twice).  Byte 0 is a
    sign crossing with about half the frame's m negative; the others are two m a power of two of bit patterns apart.  d stays
    at 0.05 or above, so no pixel takes the fill value."""
    D = np.dtype(dtype).type
    U = np.dtype(f"u{np.dtype(dtype).itemsize}").type
    rng = np.random.default_rng([seed, hw, 1])
    pair = None
    if target == TIE:
        pair = (D(3), D(3))
    elif target == 0:
        pair = (D(-3), D(3))
    else:
        base = np.array(D(3.0)).view(U)
        for j in range(8 * np.dtype(dtype).itemsize - 3):
            m2 = np.array(base + (U(1) << U(j))).view(D)
            if parting_byte(_g_of(m2), _g_of(np.array(D(3)))) == target:
                pair = (m2[()], D(3))                                    # g falls as m grows: m2 gives the lower g
                break
    assert pair is not None, (dtype, target)
    pool = (rng.uniform(0.1, 50.0, 60 * hw) * rng.choice([-1.0, 1.0], 60 * hw)).astype(D)
    m = _around_g(pair[0], pair[1], pool, hw, rng)
    d = (0.05 + 0.9 * rng.random(hw)).astype(np.float32)
    return d, m.astype(D)


def _around_g(lo, hi, pool, hw, rng):
    gp = _g_of(pool)
    nb = (hw - 1) // 2
    below, above = pool[gp < _g_of(np.array(lo))], pool[gp > _g_of(np.array(hi))]
    v = np.concatenate([below[:nb], [lo, hi], above[:hw - nb - 2]])
    assert v.size == hw
    return v[rng.permutation(hw)]


D_PAIRS = {"zero": (-0.0, 0.0), "across_zero": (-0.25, 0.25), "across_exponent": (float(np.nextafter(np.float32(2), np.float32(0))), 2.0),
           "subnormal": (1e-42, 3e-42), "subnormal_next": (1e-42, float(np.nextafter(np.float32(1e-42), np.float32(1))))}


def d_pair(dtype, target):
    """Two float32 disparities whose keys, widened to `dtype` as the kernel keys d, part at byte `target`: a power of two of bit
    patterns apart (bit 0: a nextafter pair), or a named pair of D_PAIRS."""
    if target in D_PAIRS:
        return tuple(np.float32(v) for v in D_PAIRS[target])
    if target == TIE:
        return np.float32(0.5625), np.float32(0.5625)
    base = np.array(0x3F101010, np.uint32)
    for j in range(31):
        lo, hi = base.view(np.float32), np.array(base + (np.uint32(1) << np.uint32(j))).view(np.float32)
        if parting_byte(lo.astype(dtype), hi.astype(dtype)) == target:
            return lo[()], hi[()]
    raise AssertionError((dtype, target))


def d_frame(dtype, hw, target, seed=0):
    """A frame whose disparities have the middle pair d_pair(dtype, target).  m stays at 2 or above, so no pixel takes the fill
    value whatever its d."""
    D = np.dtype(dtype).type
    rng = np.random.default_rng([seed, hw, 2])
    lo, hi = d_pair(dtype, target)
    below = (lo - np.float32(0.01) - rng.random(hw, np.float32)).astype(np.float32)
    above = (hi + np.float32(0.01) + rng.random(hw, np.float32)).astype(np.float32)
    d = _around(lo, hi, below, above, hw, rng).astype(np.float32)
    m = rng.uniform(2.0, 20.0, hw).astype(D)
    return d, m


STEPBITS = (None, 0, 4, 8, 12, 20)


def family_frame(dtype, hw, seed, stepbits, flip=False, twin=False):
    """The family that reaches the ratio's and the residual's bytes: about 40 % of the pixels share one disparity and their metric
    depths sit at consecutive bit patterns stepped by 1 << stepbits (None: one value), so that within the group the ratio and
    the residual are monotone in g; the other pixels follow m = 1 / (a d + b) with 5 % noise.  flip: half of the others get a
    negative m.  twin: two of the others sit on the line without noise, with one m and adjacent disparities, so that their ratios
    differ in the last bits only (the ratio's last float32 byte is out of the group's reach: its denominator there is 1e-8)."""
    D = np.dtype(dtype).type
    U = np.dtype(f"u{np.dtype(dtype).itemsize}")
    rng = np.random.default_rng([seed, hw, 99 if stepbits is None else stepbits, int(flip) + 2 * int(twin)])
    d = (0.05 + 0.9 * rng.random(hw)).astype(np.float32)
    a, b = rng.uniform(0.5, 2.0), rng.uniform(0.0, 0.2)
    m = (1.0 / (a * d + b) * (1 + 0.05 * rng.standard_normal(hw))).astype(D)
    perm = rng.permutation(hw)
    ng = max(2, int(0.4 * hw))
    idx, rest = perm[:ng], perm[ng:]
    d0 = np.float32(rng.uniform(0.35, 0.65))
    d[idx] = d0
    m0 = int(np.array(1.0 / (a * float(d0) + b), D).view(U))
    steps = (np.arange(ng) - ng // 2) * (0 if stepbits is None else 1 << stepbits)
    m[idx] = (m0 + steps).astype(U).view(D)
    if flip:
        m[rest[:hw // 2]] *= D(-1)
    if twin:
        dt = np.float32(rng.uniform(0.8, 0.95))
        d[rest[-2:]] = dt, np.nextafter(dt, np.float32(2))
        m[rest[-2:]] = D(1.0 / (a * float(dt) + b))
    return d, m


# (seed, stepbits, flip, twin) of family_frame at hw = 40 by the (selection, byte) its middle pair parts at, found by a search
# over 400 seeds; test_mono_limits_cpu.py recomputes every entry.  The ratio's byte 6 in float64 was not reached.
FAMILY = {
    np.float32: {("ratio", TIE): (1, None, False, False), ("ratio", 0): (159, None, False, False), ("ratio", 1): (0, None, False, False),
                 ("ratio", 2): (3, None, False, False), ("ratio", 3): (17, 0, False, True),
                 ("resid", TIE): (0, None, False, False), ("resid", 0): (167, 0, False, False), ("resid", 1): (253, None, False, False),
                 ("resid", 2): (1, 0, False, False), ("resid", 3): (0, 0, False, False)},
    np.float64: {("ratio", TIE): (1, None, False, False), ("ratio", 0): (382, 8, False, False), ("ratio", 1): (0, None, False, False),
                 ("ratio", 2): (3, None, False, False), ("ratio", 3): (37, 4, False, False), ("ratio", 4): (6, 0, False, False),
                 ("ratio", 5): (48, 20, False, False), ("ratio", 7): (323, 0, False, False),
                 ("resid", TIE): (0, None, False, False), ("resid", 0): (43, None, True, False), ("resid", 1): (76, 0, False, False),
                 ("resid", 2): (253, None, False, False), ("resid", 3): (0, 20, False, False), ("resid", 4): (32, 12, False, False),
                 ("resid", 5): (91, 4, False, False), ("resid", 6): (3, 0, False, False), ("resid", 7): (1, 0, False, False)},
}
MEDIAN_HW = (40, 41)                                                     # even: the pair's mean2; odd: one element


def d_bytes(dtype):
    """The key bytes two float32 disparities can part at once widened to `dtype`: a float32's 32 bits fill a float64 key's bits
    63..29 (sign, exponent and the upper 23 mantissa bits), bytes 0-4."""
    return range(4 if np.dtype(dtype).itemsize == 4 else 5)


def median_frames(dtype, hw):
    """[(label, claim, d [hw], m [hw])]: the constructed frames of one dtype and frame size.  claim = (selection, byte): the
    middle pair of that selection parts at that byte when hw is MEDIAN_HW[0] (test_mono_limits_cpu.py checks each); an odd hw
    builds the same frames around one middle element."""
    dtype = np.dtype(dtype).type
    out = []
    for t in [TIE] + list(range(np.dtype(dtype).itemsize)):
        out.append((f"g_{t}", ("g", t)) + g_frame(dtype, hw, t))
    for t in [TIE] + list(d_bytes(dtype)):
        out.append((f"d_{t}", ("d", t)) + d_frame(dtype, hw, t))
    for name in D_PAIRS:
        out.append((f"d_{name}", None) + d_frame(dtype, hw, name))
    for (sel, t), (seed, stepbits, flip, twin) in FAMILY[dtype].items():
        out.append((f"{sel}_{t}", (sel, t)) + family_frame(dtype, hw, seed, stepbits, flip, twin))
    return out


def median_scene(dtype, hw):
    """The constructed frames of median_frames stacked into one scene: frames of one launch part at different bytes."""
    fr = median_frames(dtype, hw)
    return np.stack([f[2] for f in fr]), np.stack([f[3] for f in fr])


# ---------------------------------------------------------------------- round P: the percentile's two ranks
def percentile_ranks(n_elems, dtype):
    """numpy's previous and next index of the 98th percentile of n_elems values of `dtype` (method 'linear'), both the last
    index when the virtual index is at or past it."""
    q = np.true_divide(98, dtype(100))
    v = (n_elems - 1) * np.asanyarray(q)
    prev = int(np.floor(v))
    if v >= n_elems - 1:
        return n_elems - 1, n_elems - 1
    return prev, min(prev + 1, n_elems - 1)


PERCENTILE_SHAPES = {"gamma_zero": (3, 17), "gamma_low": (3, 777), "gamma_high": (2, 13), "gamma_0.7": (2, 8)}   # n = 51, 2331, 26, 16
PERCENTILE_PAIRS = {"first_byte": (1.9, 2.0),                                                  # 0x3FF33333 | 0x40000000
                    "last_byte": (float(np.array(0x3FD01010, np.uint32).view(np.float32)), float(np.array(0x3FD01011, np.uint32).view(np.float32))),
                    "tied": (1.75, 1.75), "inf": (np.inf, np.inf), "wide": (0.5, 2.9)}


# seeds of the `wide` scenes at which numpy's two forms of lerp round differently (the pair is far apart: between close neighbours
# both forms round the same sum); test_mono_limits_cpu.py recomputes each
LERP_SEEDS = {(np.float32, "gamma_low"): 0, (np.float32, "gamma_0.7"): 8, (np.float32, "gamma_high"): 5,
              (np.float64, "gamma_low"): 0, (np.float64, "gamma_0.7"): 6, (np.float64, "gamma_high"): 1}


def lerp_forms(a, b, t):
    """numpy's _lerp both ways: a + (b - a) t, which it takes for t < 0.5, and b - (b - a)(1 - t)."""
    return a + (b - a) * t, b - (b - a) * (type(t)(1) - t)


def percentile_scene(shape, kind, dtype, seed=None):
    """A scene whose disparities at the percentile's two ranks (over all T hw elements) are PERCENTILE_PAIRS[kind]: the elements
    below are under 1.5 and under the pair, those above between 3 and 3.5 (`inf`: +inf, so that y is +inf from the lower rank up).  y = a_s d + a_c
    keeps d's order while a_s > 0, which m = 1 / (a d + b) gives."""
    T, hw = PERCENTILE_SHAPES[shape]
    D = np.dtype(dtype).type
    n = T * hw
    if seed is None:
        seed = LERP_SEEDS.get((D, shape), 0) if kind == "wide" else 0
    rng = np.random.default_rng([seed, n, list(PERCENTILE_PAIRS).index(kind)])
    prev, nxt = percentile_ranks(n, D)
    lo, hi = (np.float32(v) for v in PERCENTILE_PAIRS[kind])
    v = np.concatenate([(0.05 + (min(float(lo), 1.5) - 0.05) * rng.random(prev)).astype(np.float32), [lo] + [hi] * (nxt - prev),
                        np.full(n - nxt - 1, np.inf, np.float32) if kind == "inf" else (3.0 + 0.5 * rng.random(n - nxt - 1)).astype(np.float32)])
    d = v[rng.permutation(n)].astype(np.float32).reshape(T, hw)
    a, b = rng.uniform(0.5, 2.0, (T, 1)), rng.uniform(0.01, 0.2, (T, 1))
    with np.errstate(all="ignore"):
        m = (1.0 / (a * np.minimum(d, np.float32(4)) + b) * (1 + 0.02 * rng.standard_normal((T, hw)))).astype(D)
    return d, m


# ---------------------------------------------------------------------- grid-stride loops and the scene kernel
def stride_scene(T, hw, dtype, seed=0):
    """A random scene [T, hw] built without a loop over the frames: m = 1 / (a d + b) per frame with ties in d, a tenth of m at 2
    and some pixels on the fill condition."""
    D = np.dtype(dtype).type
    rng = np.random.default_rng([seed, T, hw])
    d = rng.random((T, hw), np.float32)
    grid = np.float32(1 / 16) * rng.integers(1, 16, (T, hw)).astype(np.float32)
    d = np.where(rng.random((T, hw), np.float32) < 0.3, grid, d).astype(np.float32)
    d[rng.random((T, hw), np.float32) < 0.05] = np.float32(0.02)
    a, b = rng.uniform(0.5, 2.0, (T, 1)), rng.uniform(0.01, 0.2, (T, 1))
    m = (1.0 / (a * d + b)).astype(D)
    m[rng.random((T, hw), np.float32) < 0.1] = D(2.0)
    return d, m


def scene_distances(s, c):
    """|p - median(p)| of restate's argmin, for p = s c."""
    with np.errstate(all="ignore"):
        p = s * c
        return np.abs(p - np.median(p))


def designed_scene(T, hw, dtype, k, tie=None, nan_frame=None):
    """stride_scene with the chosen frame designed: frames are independent, so swapping the argmin's frame k0 with frame `k` moves
    the restatement's choice to k.  tie: frame k is copied to that later index as well (two equal, minimal distances: the first
    wins).  nan_frame: a NaN in that frame's metric depth (s is NaN there, every distance is NaN and numpy's argmin is 0).
    The first seed whose scene has one strict minimum (before the copy) and gives the design is taken; returns d, m and the
    restatement's outputs."""
    for seed in range(64):
        d, m = stride_scene(T, hw, dtype, seed)
        _, s, c, _, k0 = restate_frames(d, m)
        dist = scene_distances(s, c)
        if np.isnan(dist).any() or (dist == dist[k0]).sum() != 1:
            continue
        for x in (d, m):
            if k is not None:
                x[[k0, k]] = x[[k, k0]]
            if tie is not None:
                x[tie] = x[k]
        if nan_frame is not None:
            m[nan_frame, hw // 2] = np.nan
        ref = restate_frames(d, m)
        dist = scene_distances(ref[1], ref[2])
        if nan_frame is not None:
            if ref[4] == 0 and np.isnan(ref[1][nan_frame]):
                return d, m, ref
        elif ref[4] == k and (dist == dist[k]).sum() == (1 if tie is None else 2) and dist[k] == dist.min():
            return d, m, ref
    raise AssertionError(("no seed gives the design", T, hw, dtype, k, tie, nan_frame))


SCENE_T = (65, 130, 1024, 1025, 1100)                                    # hw = 4, both dtypes


def scene_designs(T):
    """(k, tie, nan_frame) of the scene kernel's cases at T frames: k at 0, in the last lane of wave 0, in the first lane of wave
    1, at 1023, at 1024 (the second trip, where T allows) and at T - 1; ties with the copy in another wave and in another
    1024-trip; a NaN frame at an index above 1024."""
    ks = [j for j in (0, 63, 64, 1023, 1024, T - 1) if j < T]
    out = [(j, None, None) for j in dict.fromkeys(ks)]
    out.append((3, min(64 + 5, T - 1), None))                            # the copy in another wave
    if T > 1024:
        out.append((70, 1024 + (T - 1024) // 2, None))                   # the copy in another trip
    if T > 1026:
        out.append((None, None, 1025 + (T - 1025) // 3))
    return out


def parts_for(nseg, length, hist_threads=512, hist_target=2048):
    """mono_align.hip's parts_for: workgroups per segment of a histogram pass."""
    want, most = (hist_target + nseg - 1) // nseg, (length + 4 * hist_threads - 1) // (4 * hist_threads)
    return max(1, min(want, most))


# name: (T, hw, dtype, pointer offsets in elements): each the smallest scene that reaches the named code of mono_align.hip
STRIDE_SCENES = {
    # k_ma_pick's segment stride loop (kPickBlocks = 4096) and the second trip of k_ma_init's histogram clear (1024 x 256 threads
    # over T x 1024 words: from T = 257)
    "pick_stride": (4099, 5, np.float64, {}),
    # k_ma_hist's unit stride loop: nseg * parts past the grid cap of 65536
    "hist_grid_cap": (66000, 3, np.float32, {}),
    # the second trip of k_ma_init's Seg clear (262144 threads); about 1.07 GB of workspace
    "init_seg_trip": (262200, 2, np.float32, {}),
    # parts_for(2048, 2052) = 1: a thread's second trip in rounds A/B/C (4 x kHistThreads = 2048 elements a workgroup's trip), in
    # round P (n > 2048 x 2048) and in k_ma_write (n > kWriteBlocks x kWriteThreads x 4), 16-byte loads
    "second_trips_vector": (2048, 2052, np.float64, {}),
    # the same through the scalar kernels (512 elements a trip; round P from n > 1048576, the write from n > 524288)
    "second_trips_scalar": (2048, 2052, np.float32, {"mono_off": 1, "out_off": 1}),
    # parts_for(3, hw) = 4 workgroups a frame in float64: hw = 6151 scalar (hw % 4 != 0), 6152 vector
    "parts_scalar": (3, 6151, np.float64, {}),
    "parts_vector": (3, 6152, np.float64, {}),
}
