"""CPU half of the mono-depth alignment's limits pass (tests/test_gpu_mono_limits.py): the builders of mono_util.py checked on the
host, so that what the GPU cases claim to reach is asserted and not assumed.
  restate_frames       bit-equal to restate (the authority) on every output, both dtypes, small and long scenes, non-finite values
  constructed medians  the key byte (csrc/radix_select.hpp) at which every constructed frame's middle pair parts, recomputed from
                       the restatement's intermediates, and the coverage table over both dtypes with its explicit exemptions
  round P              gamma of the three element counts, the disparities at the percentile's two ranks, a_s > 0
  stride scenes        every scene crosses the launch constant it is named for (restated here beside the source's names)
  scene kernel         the designed k, the ties' equal minimal distances, the NaN frame's k = 0"""
import numpy as np
import pytest

from mono_util import (D_PAIRS, FAMILY, MEDIAN_HW, PERCENTILE_PAIRS, PERCENTILE_SHAPES, SCENE_T, SELECTIONS, STRIDE_SCENES, TIE, d_bytes, designed_scene,
                       fkey, frame_partings, lerp_forms, frame_values, median_frames, median_scene, middle_pair, parting_byte, parts_for,
                       percentile_gamma, percentile_ranks, percentile_scene, restate, restate_frames, scene_designs, scene_distances,
                       stride_scene)

DTYPES = [np.float32, np.float64]


def same_outputs(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x, y, equal_nan=True)
    assert a[4] == b[4]


# ---------------------------------------------------------------------- restate_frames against restate
def nonfinite_scene(dtype, seed):
    """NaN, +-inf, zeros and ties in both inputs; seed 0 keeps NaN out of mono (which would make every output NaN)."""
    rng = np.random.default_rng(40 + seed)
    T, hw = 9, 12
    d = rng.choice(np.linspace(0, 1, 7, dtype=np.float32), (T, hw)).astype(np.float32)
    m = (1.0 / (rng.uniform(0.5, 2.0, (T, 1)) * d + 0.1)).astype(dtype)
    odd = rng.random((T, hw)) < 0.15
    m[odd] = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, 2.0, -3.0], dtype), int(odd.sum()))
    m[2, :7] = 0.0
    m[3, 4] = np.nan
    d[5, 1] = np.inf
    d[6, :8] = 0.0
    if seed:
        d[7, 2] = np.nan
    return d, m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,hw", [(5, 7), (70, 6), (1500, 5), (1500, 4), (3, 1), (1, 2)])
def test_restate_frames_is_restate(T, hw, dtype):
    d, m = stride_scene(T, hw, dtype, seed=3)
    same_outputs(restate_frames(d, m), restate(d, m))
    same_outputs(restate_frames(d.reshape(T, 1, hw), m.reshape(T, 1, hw)), restate(d.reshape(T, 1, hw), m.reshape(T, 1, hw)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", [0, 1])
def test_restate_frames_is_restate_on_nonfinite_values(seed, dtype):
    d, m = nonfinite_scene(dtype, seed)
    assert np.isnan(m).any() and np.isinf(m).any() and (m == 0).any() and np.isinf(d).any() and np.unique(d).size < 10
    ref = restate(d, m)
    assert np.isnan(ref[1]).any() and (seed == 1 or not np.isnan(ref[1]).all())
    same_outputs(restate_frames(d, m), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_restate_frames_is_restate_on_the_constructed_scenes(dtype):
    for hw in MEDIAN_HW:
        d, m = median_scene(dtype, hw)
        same_outputs(restate_frames(d, m), restate(d, m))
    for shape in PERCENTILE_SHAPES:
        for kind in PERCENTILE_PAIRS:
            d, m = percentile_scene(shape if kind != "inf" else "gamma_low", kind, dtype)
            same_outputs(restate_frames(d, m), restate(d, m))


# ---------------------------------------------------------------------- keys, middle pairs, the coverage table
def test_keys_order_as_the_values_do():
    for dtype in DTYPES:
        v = np.array([-np.inf, -3.0, -1e-42, -0.0, 0.0, 1e-42, 0.5, 2.0, np.inf], dtype)
        k = fkey(v)
        assert k[3] == k[4] and (np.diff(k.astype(object)) >= 0).all() and np.unique(k).size == v.size - 1
    f = np.float32
    assert parting_byte(f(1.0), f(1.0)) == TIE and parting_byte(f(-0.0), f(0.0)) == TIE
    assert parting_byte(f(-1.0), f(1.0)) == 0 and parting_byte(f(1.0), np.nextafter(f(1.0), f(2))) == 3
    assert parting_byte(np.float64(1.0), np.nextafter(np.float64(1.0), np.float64(2))) == 7
    assert parting_byte(np.float64(1.5), np.float64(2.0)) == 0
    assert middle_pair([3.0, 1.0, 2.0]) == (2.0, 2.0) and middle_pair([4.0, 3.0, 1.0, 2.0]) == (2.0, 3.0)


def test_frame_values_restate_the_medians():
    """The intermediates the partings are read from are the restatement's: their medians are its s and c."""
    for dtype in DTYPES:
        d, m = median_scene(dtype, MEDIAN_HW[0])
        _, s, c, _, _ = restate(d, m)
        for t in range(len(d)):
            v = frame_values(d[t], m[t])
            assert all(v[name].dtype == dtype for name in SELECTIONS)
            assert np.median(v["ratio"]) == s[t] and np.median(v["resid"]) == c[t]


# (selection, dtype, byte) no builder reaches, each with its reason.  None may name g or d, a first byte, a last byte or a tie.
EXEMPT = {
    ("ratio", np.float64, 6): "400 seeds of every step width of the family part the ratio's float64 pair at bytes 0-5 and 7 only: in "
                              "the group the numerator g - median(g) + 1e-8 is dominated by 1e-8 and the ratios differ by whole "
                              "steps of g / 1e-8, outside it neighbouring ratios are unrelated",
}


@pytest.mark.parametrize("dtype", DTYPES)
def test_constructed_frames_part_where_they_claim_and_cover_the_table(dtype):
    nbytes = np.dtype(dtype).itemsize
    frames = median_frames(dtype, MEDIAN_HW[0])
    assert MEDIAN_HW[0] % 2 == 0 and MEDIAN_HW[1] % 2 == 1 and len(frames) >= 3
    reached = {name: set() for name in SELECTIONS}
    for label, claim, d, m in frames:
        part = frame_partings(d, m)
        assert None not in part.values(), label                           # no NaN in a constructed frame
        if claim is not None:
            assert part[claim[0]] == claim[1], (label, part)
        for name in SELECTIONS:
            reached[name].add(part[name])
        v = frame_values(d, m)
        lo, hi = middle_pair(v[claim[0]] if claim else v["d"])
        if claim is not None and claim[1] != TIE:
            assert lo < hi                                                 # on an even count the median is the mean of two distinct elements
    want = {"g": set(range(nbytes)) | {TIE}, "d": set(d_bytes(dtype)) | {TIE}, "ratio": {0, nbytes - 1, TIE}, "resid": {0, nbytes - 1, TIE}}
    for name in SELECTIONS:
        assert want[name] <= reached[name], (name, sorted(map(str, want[name] - reached[name])))
    for (name, dt, byte), why in EXEMPT.items():
        assert name not in ("g", "d") and byte not in (0, np.dtype(dt).itemsize - 1, TIE) and why
    for name in ("ratio", "resid"):                                       # every byte is reached or exempted by name
        for byte in range(nbytes):
            assert byte in reached[name] or (name, dtype, byte) in EXEMPT, (name, byte)
    assert all(part_sel in ("ratio", "resid") for part_sel, _ in FAMILY[dtype])
    # the named disparity pairs: a tie across zero, a sign crossing, an exponent crossing, subnormals
    for name, (lo, hi) in D_PAIRS.items():
        lo, hi = np.float32(lo), np.float32(hi)
        assert lo <= hi and (name == "zero") == (parting_byte(lo, hi) == TIE)
    tiny = np.finfo(np.float32).tiny
    assert 0 < np.float32(D_PAIRS["subnormal"][1]) < tiny and np.signbit(np.float32(D_PAIRS["zero"][0]))
    # an odd count builds around one middle element
    for label, claim, d, m in median_frames(dtype, MEDIAN_HW[1]):
        assert d.size == m.size == MEDIAN_HW[1] and m.dtype == dtype and d.dtype == np.float32


def test_float32_disparities_part_in_the_upper_five_bytes_of_a_float64_key():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)
    v = bits.view(np.float32)
    v = v[np.isfinite(v)].astype(np.float64)
    assert ((fkey(v) & np.uint64((1 << 29) - 1)) == np.where(v < 0, np.uint64((1 << 29) - 1), np.uint64(0))).all()
    assert list(d_bytes(np.float64)) == [0, 1, 2, 3, 4] and list(d_bytes(np.float32)) == [0, 1, 2, 3]


# ---------------------------------------------------------------------- round P
@pytest.mark.parametrize("dtype", DTYPES)
def test_percentile_scenes_have_the_gamma_and_the_neighbours_they_claim(dtype):
    sizes = {s: T * hw for s, (T, hw) in PERCENTILE_SHAPES.items()}
    assert sizes == {"gamma_zero": 51, "gamma_low": 2331, "gamma_high": 26, "gamma_0.7": 16}
    assert percentile_gamma(51, dtype) == 0.0 and 0.0 < percentile_gamma(2331, dtype) < 0.5 <= percentile_gamma(26, dtype) < 1.0
    assert 0.69 < percentile_gamma(16, dtype) < 0.71 and sum(n % 4 == 0 for n in sizes.values()) == 1
    assert percentile_ranks(1, dtype) == (0, 0) and percentile_ranks(2, dtype) == (0, 1)
    f = np.float32
    assert parting_byte(*map(f, PERCENTILE_PAIRS["first_byte"])) == 0 and parting_byte(*map(f, PERCENTILE_PAIRS["last_byte"])) == 3
    for shape, n in sizes.items():
        for kind, pair in PERCENTILE_PAIRS.items():
            if kind == "inf" and shape != "gamma_low":
                continue
            d, m = percentile_scene(shape, kind, dtype)
            assert d.size == n and m.dtype == dtype
            prev, nxt = percentile_ranks(n, dtype)
            assert nxt == prev + 1
            v = np.sort(d.ravel())
            assert (v[prev], v[nxt]) == (f(pair[0]), f(pair[1])) and (prev == 0 or v[prev - 1] < v[prev]) and (nxt == n - 1 or v[nxt + 1] >= v[nxt])
            depth, _, _, aligns, k = restate(d, m)
            assert aligns[0] > 0                                           # y = a_s d + a_c keeps d's order
            with np.errstate(all="ignore"):
                y = np.sort((aligns[0] * d + aligns[1]).ravel())
            if kind == "inf":
                assert np.isposinf(y[prev:]).all() and np.isfinite(y[:prev]).all() and np.isnan(aligns[2]) and np.isnan(depth).all()
            else:
                assert np.isfinite(aligns).all() and (kind != "first_byte" or y[prev] < y[nxt]) and (kind != "tied" or y[prev] == y[nxt])
            if kind == "wide" and shape != "gamma_zero":                   # a kernel with one form of lerp gives another value here
                one, other = lerp_forms(y[prev], y[nxt], dtype(percentile_gamma(n, dtype)))
                assert one != other and aligns[2] == (one if percentile_gamma(n, dtype) < 0.5 else other) / dtype(2)


# ---------------------------------------------------------------------- the launch constants (csrc/mono_align.hip)
HIST_THREADS, HIST_GRID_CAP = 512, 65536                                  # kHistThreads; grid_for(nseg * parts, 65536)
PICK_BLOCKS = 4096                                                        # kPickBlocks
SCENE_THREADS = 1024                                                      # kSceneThreads
WRITE_THREADS, WRITE_BLOCKS = 256, 2048                                   # kWriteThreads, kWriteBlocks
INIT_THREADS, HIST_WORDS = 1024 * 256, 4 * 256                            # k_ma_init's grid cap x block; kMaxSel * kBins words a frame

def test_stride_scenes_cross_their_thresholds():
    assert parts_for(50, 480 * 854) == 41 and parts_for(64, 777) == 1 and parts_for(1, 1) == 1 and parts_for(1, 1 << 30) == 2048
    # the scene kernel: waves 1..15 from T = 65, the second trip of both loops past 1024
    assert SCENE_T[0] == 64 + 1 and max(t for t in SCENE_T if t <= SCENE_THREADS) == SCENE_THREADS and SCENE_THREADS + 1 in SCENE_T
    assert 130 in SCENE_T and 130 > 2 * 64                                # three waves carry frames
    per = lambda scalar: HIST_THREADS * (1 if scalar else 4)               # elements a workgroup's first trip takes
    T, hw, _, _ = STRIDE_SCENES["pick_stride"]
    assert T > PICK_BLOCKS and T * HIST_WORDS > INIT_THREADS and 256 * HIST_WORDS == INIT_THREADS   # the init clear's second trip from T = 257
    T, hw, _, _ = STRIDE_SCENES["hist_grid_cap"]
    assert T * parts_for(T, hw) > HIST_GRID_CAP and hw <= 2048
    T, hw, _, _ = STRIDE_SCENES["init_seg_trip"]
    assert T > INIT_THREADS and T * 4096 > 1 << 30                         # about 1.07 GB of histograms
    for name in ("second_trips_vector", "second_trips_scalar"):
        T, hw, dtype, offsets = STRIDE_SCENES[name]
        scalar = bool(offsets)
        assert scalar == (name == "second_trips_scalar") and (not scalar or offsets == {"mono_off": 1, "out_off": 1})
        n = T * hw
        assert (hw % 4 == 0) and parts_for(T, hw) * per(scalar) < hw       # rounds A/B/C: a thread's second trip
        assert parts_for(1, n) * per(scalar) < n                           # round P
        assert WRITE_BLOCKS * WRITE_THREADS * (1 if scalar else 4) < n     # k_ma_write
    assert 2048 * 4 * HIST_THREADS == 4194304 and 2048 * HIST_THREADS == 1048576 and WRITE_BLOCKS * WRITE_THREADS == 524288
    for name, vec in (("parts_scalar", False), ("parts_vector", True)):
        T, hw, dtype, offsets = STRIDE_SCENES[name]
        assert not offsets and parts_for(T, hw) == 4 and (hw % 4 == 0) == vec and dtype == np.float64 and parts_for(T, hw - 8) == 3


# ---------------------------------------------------------------------- the scene kernel's designed k
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", SCENE_T)
def test_scene_designs_choose_the_frame_they_name(T, dtype):
    designs = scene_designs(T)
    ks = [k for k, tie, nan in designs if tie is None and nan is None]
    assert ks == [j for j in (0, 63, 64, 1023, 1024) if j < T - 1] + [T - 1]
    for k, tie, nan_frame in designs:
        d, m, ref = designed_scene(T, 4, dtype, k, tie, nan_frame)
        full = restate(d, m)
        same_outputs(ref, full)
        dist = scene_distances(full[1], full[2])
        if nan_frame is not None:
            assert nan_frame > SCENE_THREADS and np.isnan(full[1][nan_frame]) and np.isnan(dist).all() and full[4] == 0
            continue
        assert full[4] == k and dist[k] == dist.min()
        if tie is None:
            assert (dist == dist[k]).sum() == 1
        else:
            assert tie > k and tie // 64 != k // 64 and dist[tie] == dist[k] and (dist == dist[k]).sum() == 2
            assert (d[tie] == d[k]).all() and (m[tie] == m[k]).all()
    if T > SCENE_THREADS:
        assert any(tie is not None and tie >= SCENE_THREADS > k for k, tie, _ in designs)          # the copy in another 1024-trip
