"""What a shifted clone of a plan must hold (bt_plan_create_shifted{,_any,_spec}, bt_plan_preshift: csrc/plan_pack.hip), stated in
numpy from the source plan's tables alone, and the edge lists whose plans take every layout the planner has.  Shared by
tests/test_shift_tables_cpu.py (the planner is shift-equivariant on these lists: what the comparison of a clone with a freshly
planned plan rests on) and tests/test_gpu_shift_tables.py (the clones themselves).  No GPU here.

A list L moved by (df, dk) is (ii + df, jj + df, kk + dk) with fixedp + df: the caller's sliding window one update later."""
from collections import namedtuple

import numpy as np

from batrack_amd import graphgen
from batrack_amd.plan import PLAN_ARRAYS

# tables of the host's analysis that are in no device buffer and that no kernel reads: a clone has none (bt_plan_array answers
# from the clone's empty vectors), a host plan of the moved list has them moved
HOST_ONLY = ("trk_of_patch", "trk_loc")
DEVICE_TABLES = tuple(n for n in PLAN_ARRAYS if n not in HOST_ONLY)
INFO_MOVES = ("fixedp", "n_all")                       # the two figures of bt_plan_info that a shift changes


# ------------------------------------------------------------------ the reference
def popcount32(words):
    w = np.ascontiguousarray(words, np.uint32)
    return np.unpackbits(w.view(np.uint8)).reshape(-1, 32).sum(1).astype(np.int64)


def shift_bits(words, dk):
    """The bitmap `words` (uint32, bit p = word p >> 5, bit p & 31) as ONE integer moved up by dk bits, cut to the same word count"""
    w = np.ascontiguousarray(words, np.uint32)
    if w.size == 0:
        return w.copy()
    v = int.from_bytes(w.astype("<u4").tobytes(), "little") << int(dk)
    v &= (1 << (32 * w.size)) - 1
    return np.frombuffer(v.to_bytes(4 * w.size, "little"), dtype="<u4").astype(np.uint32)


def rank_of(words):
    """exclusive cumulative popcount: set bits below each word"""
    c = popcount32(words)
    return (np.cumsum(c) - c).astype(np.int32)


def expected_clone(src, df, dk):
    """{name: array} of what a clone of the plan with tables `src` holds after a shift by df frames and dk patches.  `src` may
    hold "edge_words" (the kept packed list) and the host-only tables; what it does not hold is not in the result."""
    df, dk = int(df), int(dk)
    out = {}
    for name, a in src.items():
        a = np.asarray(a)
        if name == "kx":
            b = a + np.int32(dk)
        elif name == "tile_kx":
            b = np.where(a >= 0, a + np.int32(dk), a).astype(a.dtype)
        elif name == "tile_ij":
            b = a + np.int32(df * 65537)                     # both 16-bit halves, padding included (the kernel shifts every entry)
        elif name in ("pair_i", "pair_j"):
            b = a + np.int32(df)
        elif name == "act_bits":
            b = shift_bits(a, dk)
        elif name == "act_rank":
            b = rank_of(shift_bits(src["act_bits"], dk)) if a.size else a.copy()
        elif name == "edge_words":
            b = a + np.uint64((dk << 32) | (df << 16) | df)
        elif name == "trk_of_patch":                         # host only: track of patch p, over the whole patch buffer
            b = np.full_like(a, -1)
            b[dk:] = a[:a.size - dk]
        else:
            b = a.copy()
        assert b.dtype == a.dtype and b.shape == a.shape, name
        out[name] = b
    return out


def valid_mask(arrays, name):
    """Boolean mask over arrays[name]: the entries some kernel reads.  Everything, except tile_ij — [tiles][max_tile_pairs], of which
    a tile's kernels read the first tile_npair[t]: the planner leaves the rest 0, a clone's shift moves it too."""
    a = np.asarray(arrays[name])
    if name != "tile_ij" or a.size == 0:
        return np.ones(a.shape, bool)
    npair = np.asarray(arrays["tile_npair"])
    row = a.size // npair.size
    assert row * npair.size == a.size and npair.max() <= row
    return (np.arange(row)[None, :] < npair[:, None]).reshape(-1)


def differing(a, b, names, mask_from=None):
    """names whose tables differ between the dicts a and b (dtype, shape or any entry — under valid_mask(mask_from) if given)"""
    bad = []
    for n in names:
        x, y = np.asarray(a[n]), np.asarray(b[n])
        if x.dtype != y.dtype or x.shape != y.shape:
            bad.append((n, "shape", x.shape, y.shape))
            continue
        m = valid_mask(mask_from, n) if mask_from is not None else np.ones(x.shape, bool)
        d = np.flatnonzero((x != y) & m)
        if d.size:
            bad.append((n, int(d.size), int(d[0]), x[d[0]].item(), y[d[0]].item()))
    return bad


def edge_words(ii, jj, kk):
    return (np.asarray(kk).astype(np.uint64) << np.uint64(32)) | (np.asarray(ii).astype(np.uint64) << np.uint64(16)) | np.asarray(jj).astype(np.uint64)


def track_of(bits, rank, p):
    """track(p) = act_rank[p >> 5] + popcount(bits below p), as the kernels compute it (ba_plan.hpp: PlanDev::act_rank)"""
    p = np.asarray(p, np.int64)
    below = np.asarray(bits, np.uint32)[p >> 5] & ((np.uint32(1) << (p & 31).astype(np.uint32)) - np.uint32(1))
    return np.asarray(rank, np.int64)[p >> 5] + popcount32(below)


# ------------------------------------------------------------------ the lists
# M: patches per frame of the caller's buffers (p_tot = n_buf * M: what bt_plan_preshift and the speculative clone derive dk
# from); kernel / solver / device: the route the plan must take on the GPU; layout(arrays, info): the same stated on the
# host plan's tables (no GPU)
Fixture = namedtuple("Fixture", "name ii jj kk n_buf p_tot fixedp M kernel solver device layout")
SLACK = 8                                              # every list leaves this many frames of its buffers free


def _fx(name, ii, jj, kk, fixedp, M, kernel, solver, device, layout, n_buf=None):
    ii, jj, kk = (np.ascontiguousarray(a, np.int64) for a in (ii, jj, kk))
    n_all = int(max(ii.max(), jj.max())) + 1
    n_buf = n_all + SLACK if n_buf is None else n_buf
    assert n_buf >= n_all + SLACK and int(kk.max()) + 3 * M < n_buf * M      # (the tests shift by 1 and 3 frames at least)
    return Fixture(name, ii, jj, kk, n_buf, n_buf * M, int(fixedp), int(M), kernel, solver, device, layout)


def moved(fx, df, dk=None):
    """(ii, jj, kk, fixedp) of the fixture's list moved by df frames (dk patches: df * M unless given)"""
    dk = df * fx.M if dk is None else dk
    return fx.ii + df, fx.jj + df, fx.kk + dk, fx.fixedp + df


def _pair_major(A, I):
    return A["pm_edge"].size > 0 and A["pm_rec"].size == 4 * I["tiles"] and A["lz_trk"].size == 0


def _tile(A, I):
    return A["slot_edge"].size == 64 * I["slots"] and A["pm_edge"].size == 0 and A["it_edge"].size == 0 and I["tiles"] < 2048 and A["lz_trk"].size == 0


def _slot_uniform(A, I):
    return I["tiles"] >= 2048 and A["it_edge"].size > 0 and A["tile_sinfo"].size == 64 * I["tiles"]


def _ragged_many(A, I):
    return I["tiles"] >= 2048 and A["it_edge"].size == 0 and A["slot_code"].size == 64 * I["slots"]


def _loose(A, I):
    return A["lz_trk"].size == 3 and A["lz_ptr"][-1] == A["lz_edge"].size == 3 * 69


def _wide(A, I):
    n = I["n"]
    return n > 0 and I["nnz_blocks"] == n * (n + 1) // 2 and np.array_equal(A["perm"], np.arange(n)) and A["row_idx"].size == 0


def _window(n_frames, M):
    g, fixedp = graphgen.make_window_graph(n_frames=n_frames, M=M, seed=4, n_buf=n_frames + SLACK)
    return g.ii, g.jj, g.kk, fixedp


def etile_dev():
    return _fx("etile_dev", *_window(50, 256), 256, "k_etile", 0, True, _pair_major)


def etile_host():
    # (a window of 8 frames: the 16-track tiles of k_etile hold at most 64 camera pairs; 11 patches a frame: tiles run across
    #  source frames, and three frames are 33 patches — a word and a bit of the track bitmap)
    g, fixedp = graphgen.make_window_graph(n_frames=30, M=11, window=8, seed=4, n_buf=30 + SLACK)
    assert g.ii.size < 4096                                 # (the device planner starts at 4096 edges)
    return _fx("etile_host", g.ii, g.jj, g.kk, fixedp, 11, "k_etile", 0, False, _pair_major)


def M40():
    return _fx("M40", *_window(30, 40), 40, "k_etile", 0, True, lambda A, I: _pair_major(A, I) and (3 * 40) % 32 != 0)


def tile():
    g = graphgen.make_graph(32, 256, 8, seed=5)
    assert (g.ii == g.jj).any()                             # self edges (PlanDev::em_self)
    return _fx("tile", g.ii, g.jj, g.kk, 1, 256, "k_tile", 0, True, _tile)


def tile_repeats():
    g = graphgen.make_graph(32, 256, 8, seed=5)
    rng = np.random.default_rng(3)
    extra = rng.integers(0, g.ii.size, g.ii.size // 2)      # repeated observations, any order
    ii, jj, kk = (np.concatenate([a, a[extra]]) for a in (g.ii, g.jj, g.kk))
    p = rng.permutation(ii.size)
    return _fx("tile_repeats", ii[p], jj[p], kk[p], 1, 256, "k_tile", 0, True, _tile)


def edge2():
    g = graphgen.make_graph(64, 2048, 8, seed=0)
    return _fx("edge2", g.ii, g.jj, g.kk, 1, 2048, "k_edge2", 0, True, _slot_uniform)


def stream():
    """tests/test_gpu_device_planner.py's ragged many-tile lists (odd seed: a track's targets thinned one by one), unsharded"""
    rng = np.random.default_rng(901)
    n_frames, M, span = 28, 6144, 2
    src = np.repeat(np.arange(n_frames), M)
    pat = src * M + np.tile(np.arange(M), n_frames)
    alive = rng.random(pat.size) < 0.97
    src, pat = src[alive], pat[alive]
    off = np.arange(-span, span + 1)
    off = off[off != 0]
    tg = src[:, None] + off[None, :]
    ok = (tg >= 0) & (tg < n_frames) & (rng.random(tg.shape) < 0.8)
    ii, kk, jj = np.broadcast_to(src[:, None], tg.shape)[ok], np.broadcast_to(pat[:, None], tg.shape)[ok], tg[ok]
    # every 997th track observes each of its targets 20 times over: tiles of more than 64 slots, which the edge-major layout of
    # k_edge2 does not hold (ba_plan.cpp: aligned slots) — the plan is laid out for k_stream
    deep = np.flatnonzero(kk % 997 == 0)
    ii, jj, kk = (np.concatenate([a, np.repeat(a[deep], 19)]) for a in (ii, jj, kk))
    p = rng.permutation(ii.size)
    return _fx("stream", ii[p], jj[p], kk[p], 2, M, "k_stream", 0, True, _ragged_many)


def loose():
    """tests/mask_problems.py's hub tracks (three tracks seen from 69 frames: in no tile), in buffers with slack: 78 frames of 4
    patches, the hubs at patches 280 .. 282 — the largest shift the buffers admit is bounded by the PATCH buffer (7 frames)"""
    import mask_problems
    d, _ = mask_problems.problem("loose")
    return _fx("loose", d["ii"], d["jj"], d["kk"], 1, 4, "k_tile", 3, False, _loose)     # (69 free poses of full coupling: the dense solver too)


def wide_band():
    g = graphgen.make_graph(300, 16, 6, seed=21)            # 299 free poses: beyond the block-sparse solvers' 255
    return _fx("wide_band", g.ii, g.jj, g.kk, 1, 16, "k_tile", 3, True, _wide)


def wide_filled():
    from edge_problems import band_120
    ii, jj, kk, N, P = band_120(filled=True)                # every block fills in: the factor does not fit LDS
    return _fx("wide_filled", ii, jj, kk, 1, P // N, "k_tile", 3, False, _wide)         # (targets anywhere: beyond the device planner's masks)


FIXTURES = {f.__name__: f for f in (etile_dev, etile_host, tile, tile_repeats, edge2, stream, loose, wide_band, wide_filled, M40)}
_BUILT = {}


def fixture(name):
    """FIXTURES[name](), built once per process; treat as read-only"""
    if name not in _BUILT:
        _BUILT[name] = FIXTURES[name]()
    return _BUILT[name]


def max_shift(fx):
    """the largest df that bt_plan_preshift admits: n_all + df <= n_buf and k_hi + df * M < p_tot"""
    n_all = int(max(fx.ii.max(), fx.jj.max())) + 1
    return min(fx.n_buf - n_all, (fx.p_tot - 1 - int(fx.kk.max())) // fx.M)


# ------------------------------------------------------------------ something to step
def step_inputs(ii, jj, kk, n_buf, p_tot, seed=0):
    """float32 state and targets for an edge list: cameras a hundredth of a unit apart along a slow curve, patches 1.7 .. 5
    units deep, targets the reprojection of the unperturbed state plus half a pixel -> dict of numpy arrays"""
    rng = np.random.default_rng(seed)
    cam = graphgen.SINTEL
    f = np.arange(n_buf, dtype=np.float64)[:, None]
    gt = graphgen.se3_exp(f * np.array([0.005, 0.0, 0.01, 0.0, 0.001, 0.0]))
    pert = rng.normal(0.0, 0.003, (n_buf, 6))
    poses = graphgen.se3_mul(graphgen.se3_exp(pert), gt)
    patches = np.stack([rng.uniform(20.0, cam["wd"] - 20.0, p_tot), rng.uniform(20.0, cam["ht"] - 20.0, p_tot), rng.uniform(0.2, 0.6, p_tot)], 1)
    intr = np.tile(np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]]), (n_buf, 1))
    u, v, _ = graphgen.reproject(gt, patches, intr, ii, jj, kk)
    E = len(ii)
    t3 = np.stack([u + rng.normal(0, 0.5, E), v + rng.normal(0, 0.5, E), patches[kk, 2]], 1)
    noisy = patches.copy()
    noisy[:, 2] *= 1.0 + rng.normal(0.0, 0.05, p_tot)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(poses=f32(poses), patches=f32(noisy), mono=f32(patches[:, 2]), intrinsics=f32(intr), targets3=f32(t3),
                weights=f32(rng.uniform(0.5, 1.0, (E, 2))), bounds=(0.0, 0.0, float(cam["wd"]), float(cam["ht"])))
