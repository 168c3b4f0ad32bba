"""The reference's align_depth_maps (main/global_refine/model/utils.py:268-312) restated with its branch decisions exposed: the
aligned channel 0 and, per frame, what bt_align_depth_maps reports (include/batrack_depth.h) — `scales` (s widened to float64,
NaN for frame 0 and skipped frames), `overlap` (c, 0 for frame 0) — plus the size of the union med_prev is taken over.

Also the scenes of the limit tests (test_gpu_depth_limits.py, test_depth_limits_cpu.py): frames whose medians' middle pairs part
at a chosen byte, frames whose positive pixels lie past a kernel's first grid-stride trip, and the random sweep."""
import functools

import numpy as np

from depth_util import middle_pair_keys


def host_align_stats(ch0):
    ch0 = np.asarray(ch0)
    T = ch0.shape[0]
    out = np.zeros_like(ch0)
    out[0] = ch0[0]
    scales, overlap, union = np.full(T, np.nan), np.zeros(T, np.int64), np.zeros(T, np.int64)
    with np.errstate(all="ignore"):
        for i in range(1, T):
            prev, cur = out[i - 1], ch0[i]
            mask = (prev > 0) & (cur > 0)
            overlap[i] = mask.sum()
            if overlap[i] < 100:
                out[i] = cur
                continue
            if i == 1:
                pv = prev[mask]
            else:
                past = out[i - 2]
                pv = np.concatenate((past[(past > 0) & (prev > 0)], prev[mask]))
            union[i] = pv.size
            s = np.median(pv) / np.median(cur[mask])
            scales[i] = float(s)
            out[i] = s * cur
    return out, scales, overlap, union


# ---------------------------------------------------------------------- constructed medians
def _uint(dtype):
    return np.dtype(f"u{np.dtype(dtype).itemsize}")


def positive_pair(dtype, b, kind="normal"):
    """Bit patterns (lo, hi) of two positive values of the dtype that first differ at byte b (0 = most significant) of the raw
    bits, the kernel's key for values > 0.  kind "tied": lo == hi; "subnormal": both subnormal (b in the lower half)."""
    nb = np.dtype(dtype).itemsize
    base = 0x3F9A5C3D if nb == 4 else 0x3FF3A5C79B2D4E61
    if kind == "subnormal":
        assert b >= nb // 2
        lo = 2
        return lo, lo | (1 << (8 * (nb - 1 - b)))
    if kind == "tied":
        return base, base
    shift = 8 * (nb - 1 - b)
    keep = base & ~((1 << (shift + 8)) - 1)                               # the bytes above b
    lo_b, hi_b = (0x3F, 0x40) if b == 0 else (0x41, 0x42)
    return keep | (lo_b << shift) | (base & ((1 << shift) - 1)), keep | (hi_b << shift) | ((base >> 3) & ((1 << shift) - 1))


def positive_values(dtype, lo, hi, n, rng):
    """[n] positive finite-or-inf values of the dtype whose two middle elements have the bit patterns (lo, hi)."""
    nb = np.dtype(dtype).itemsize
    kmax = 0x7F800000 if nb == 4 else 0x7FF0000000000000                  # +inf: the largest value that passes `> 0`
    return middle_pair_keys(lo, hi, n, 1, kmax, rng).astype(_uint(dtype)).view(dtype)


_NONPOS = (0.0, -0.0, -1.0, -np.inf, np.nan, -1e-30)


def constructed_scene(dtype, hw, c, u0, cur_pair, prev_pair, seed):
    """maps [3, hw]: frame 1 overlaps frame 0 in u0 < 100 pixels, so it is skipped and aligned[1] = maps[1]; frame 2 overlaps it in
    c pixels whose values have the middle pair cur_pair, and its prev set — u0 values of frame 0 and c of frame 1 — has the middle
    pair prev_pair.  The other hw - c pixels hold a non-positive value or NaN in one frame and an extreme positive one in the
    others, which would move a median if the masks let it in."""
    assert u0 < 100 and u0 <= c <= hw
    rng = np.random.default_rng(seed)
    maps = np.empty((3, hw), dtype)
    pix = rng.permutation(hw)
    M, rest = pix[:c], pix[c:]
    cur = positive_values(dtype, cur_pair[0], cur_pair[1], c, rng)
    prev = positive_values(dtype, prev_pair[0], prev_pair[1], u0 + c, rng) if c else np.zeros(u0, dtype)
    big, tiny = np.finfo(dtype).max, np.finfo(dtype).smallest_subnormal
    maps[0] = rng.choice(np.array(_NONPOS, dtype), hw)                    # frame 0: positive at u0 pixels of M only ...
    maps[0, M[:u0]] = prev[:u0] if c else big
    maps[1, M] = prev[u0:] if c else big
    maps[2, M] = cur
    for i in rest:                                                        # ... and at pixels where frame 1 is not
        bad = rng.integers(1, 3)
        vals = rng.choice(np.array([big, tiny, np.inf], dtype), 3)
        vals[bad] = rng.choice(np.array(_NONPOS, dtype))
        if bad == 2:
            vals[0] = rng.choice(np.array(_NONPOS, dtype))               # frame 1 positive here: keep it out of the past set
        maps[:, i] = vals
    return maps


def constructed_pair_scene(dtype, hw, c, cur_pair, prev_pair, seed):
    """maps [2, hw]: frame 1 (no past frame) overlaps frame 0 in c pixels; cur and prev have the chosen middle pairs."""
    rng = np.random.default_rng(seed)
    big = np.finfo(dtype).max
    maps = np.empty((2, hw), dtype)
    pix = rng.permutation(hw)
    maps[0, pix[:c]] = positive_values(dtype, prev_pair[0], prev_pair[1], c, rng)
    maps[1, pix[:c]] = positive_values(dtype, cur_pair[0], cur_pair[1], c, rng)
    for i in pix[c:]:
        bad = rng.integers(0, 2)
        maps[bad, i], maps[1 - bad, i] = rng.choice(np.array(_NONPOS, dtype)), big
    return maps


def constructed_cases(dtype, hw):
    """(label, maps, c of the last frame, its union count, cur byte, prev byte): every byte of the dtype for cur with another one
    for prev, crossed with c and the union count odd and even; a tied and a subnormal pair; c = 99 (skipped), 100 and 101."""
    nb = np.dtype(dtype).itemsize
    out = []
    seed = 0
    for b in range(nb):
        pb = (b + 1) % nb
        for c in (100, 101):
            for u0 in (7, 8):
                if c > hw:
                    continue
                seed += 1
                maps = constructed_scene(dtype, hw, c, u0, positive_pair(dtype, b), positive_pair(dtype, pb), 1000 * hw + seed)
                out.append((f"b{b}/p{pb}/c{c}/u{u0}", maps, c, u0 + c, b, pb))
    for kind, b, pb in (("tied", None, 0), ("subnormal", nb - 1, nb // 2), ("subnormal", nb // 2, nb - 1)):
        for c, u0 in ((100, 7), (100, 8)) + (((101, 8),) if hw >= 101 else ()):
            seed += 1
            cur = positive_pair(dtype, b, kind)
            prev = positive_pair(dtype, pb, "subnormal" if kind == "subnormal" else "normal")
            out.append((f"{kind}/b{b}/p{pb}/c{c}/u{u0}", constructed_scene(dtype, hw, c, u0, cur, prev, 1000 * hw + seed), c, u0 + c, b, pb))
    for c in (99, 100) + ((101,) if hw >= 101 else ()):
        seed += 1
        out.append((f"threshold/c{c}", constructed_scene(dtype, hw, c, 9, positive_pair(dtype, 1), positive_pair(dtype, 2), 1000 * hw + seed),
                    c, 9 + c, 1, 2))
    for b in range(nb):                                                   # frame 1 of two: prev = aligned[0][m], no union
        for c in (100,) + ((101,) if hw >= 101 else ()):
            seed += 1
            pb = (b + 2) % nb
            maps = constructed_pair_scene(dtype, hw, c, positive_pair(dtype, b), positive_pair(dtype, pb), 1000 * hw + seed)
            out.append((f"two/b{b}/p{pb}/c{c}", maps, c, c, b, pb))
    return out


# ---------------------------------------------------------------------- a second trip of the grid-stride loops
# depth_align.hip:28-29: kHistThreads = 512, kHistBlocks = 256; kWriteThreads = 256, kWriteBlocks = 1024.  A thread takes one
# 16-byte vector (4 float32, 2 float64) per trip on the vectorised path, one pixel on the scalar path.
HIST_THREADS, WRITE_THREADS = 512 * 256, 256 * 1024
# (dtype, hw, elements the base is offset by, pixels per thread per trip)
SECOND_TRIP = [(np.float32, 1_050_628, 0, 4), (np.float64, 525_314, 0, 2), (np.float32, 263_169, 0, 1), (np.float64, 263_169, 0, 1),
               (np.float32, 263_172, 1, 1)]


@functools.lru_cache(maxsize=None)
def second_trip_scene(dtype, hw, per_thread):
    """(maps [4, hw], host_align_stats of it): frame 2 is positive only at or past the histogram pass's first trip
    (HIST_THREADS * per_thread pixels); the other frames are positive nearly everywhere."""
    rng = np.random.default_rng(hw)
    maps = rng.uniform(0.5, 4.0, (4, hw)).astype(dtype)
    maps[rng.random((4, hw)) < 0.02] = 0.0
    first = HIST_THREADS * per_thread
    maps[2, :first] = rng.choice(np.array([0.0, -0.0, -2.0, np.nan], dtype), first)
    maps.setflags(write=False)
    ref = host_align_stats(maps)
    for a in ref:
        a.setflags(write=False)
    return maps, ref


# ---------------------------------------------------------------------- the random sweep
SWEEP_SEEDS = range(24)
SWEEP_T, SWEEP_HW = (2, 3, 9), (100, 101, 102, 103, 511, 512, 513, 2049)


def sweep_scene(seed, dtype):
    """maps [T, hw], T = SWEEP_T[seed % 3], hw = SWEEP_HW[seed // 3]: values from a tie-heavy pool mixed with uniforms; 0, -0,
    negatives, +-inf and NaN sprinkled over slots few enough to leave 100 overlapping pixels; and sparse frames (fewer than 100
    positive pixels), after which the chain skips twice and scales again."""
    T, hw = SWEEP_T[seed % 3], SWEEP_HW[seed // 3]
    rng = np.random.default_rng(7000 + seed)
    x = rng.choice(np.linspace(0.25, 4.0, 16), (T, hw))
    x = np.where(rng.random((T, hw)) < 0.5, rng.uniform(0.1, 5.0, (T, hw)), x)
    slots = rng.permutation(hw)[:min(hw - 100, hw // 12)]                 # every overlap outside them: c >= 100
    odd = np.array([0.0, -0.0, -1.5, -np.inf, np.nan, np.inf, np.inf])
    for t in range(T):
        use = slots[rng.random(slots.size) < 0.6]
        x[t, use] = rng.choice(odd, use.size)
    sparse = {2: (1,) if (seed // 3) % 2 else (), 3: ((), (1,), (2,))[(seed // 3) % 3], 9: (3, 6)}[T]
    for t in sparse:
        keep = rng.integers(0, 100)
        x[t, rng.permutation(hw)[keep:]] = rng.choice(odd[:5], hw - keep)
    return x.astype(dtype)
