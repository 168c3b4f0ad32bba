"""Edge lists for tools/plan_dump.cpp, from the generators the tests use.

    python tools/plan_corpus.py corpus.bin            the parity corpus (prints index and name of every case)
    python tools/plan_corpus.py timing.bin --timing   C3, the 50 x 256 window, the 64 x 16384 x 8 graph

A case: int64 E, n_buf, p_tot, fixedp, n_all_min, own_lo, own_hi, then ii, jj, kk (int64)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from batrack_amd import graphgen  # noqa: E402
from batrack_amd.parallel import partition_tracks, plan_range  # noqa: E402
import edge_problems  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def chain(N, K=3):
    """tests/test_plan_cpu.py: _chain_edges"""
    kk = np.repeat(np.arange(N, dtype=np.int64), K)
    return kk.copy(), np.clip(kk + np.tile(np.arange(1, K + 1, dtype=np.int64), N), 0, N - 1), kk


def ragged(ii, jj, kk, drop, seed=11, repeat=0.0):
    """a random share of the observations dropped, another share repeated"""
    rng = np.random.default_rng(seed)
    keep = rng.random(kk.size) > drop
    ii, jj, kk = ii[keep], jj[keep], kk[keep]
    if repeat:
        again = np.nonzero(rng.random(kk.size) < repeat)[0]
        ii, jj, kk = (np.concatenate([a, a[again]]) for a in (ii, jj, kk))
    return ii, jj, kk


def deep(N, M, span, times):
    """M tracks per frame, each seen `times` times from the `span` frames around its source: deep edge lists, few tiles"""
    kk = np.repeat(np.arange(N * M, dtype=np.int64), span * times)
    ii = kk // M
    jj = np.clip(ii + np.tile(np.repeat(np.arange(span, dtype=np.int64) - span // 2, times), N * M), 0, N - 1)
    return ii, jj, kk


def with_track(ii, jj, kk, k, src, targets):
    t = np.asarray(targets, np.int64)
    return np.concatenate([ii, np.full(t.size, src)]), np.concatenate([jj, t]), np.concatenate([kk, np.full(t.size, k)])


def cases():
    out = []

    def add(name, ii, jj, kk, n_buf, p_tot, fixedp, n_all_min=0, own=(0, 0)):
        out.append((name, [np.ascontiguousarray(np.asarray(a, np.int64)) for a in (ii, jj, kk)], int(n_buf), int(p_tot), int(fixedp), int(n_all_min), own))

    def add_graph(name, g, fixedp, **kw):
        add(name, g.ii, g.jj, g.kk, g.poses.shape[0], g.patches.shape[0], fixedp, **kw)

    # goldens and standard graphs
    for name, fps in (("c1", (1, 3, 8)), ("c1_rough", (1, 2)), ("window_small", (None,))):
        d = np.load(os.path.join(GOLD, name + ".npz"))
        for fp in fps:
            add(f"{name} fixedp={fp}", d["ii"], d["jj"], d["kk"], d["poses"].shape[0], d["patches"].shape[0], int(d["fixedp"]) if fp is None else fp)
    add_graph("C3", graphgen.make_config("C3", seed=0), 1)
    g, fp = graphgen.make_window_graph(n_frames=50, M=256, seed=4)
    add_graph("window 50x256", g, fp)
    for r, own in enumerate(partition_tracks(g.kk, 2)):
        add_graph(f"window 50x256 rank {r}/2", g, fp, own=plan_range(own, g.patches.shape[0]))
    for seed, N, M, fixedp, far, groups in [(0, 10, 6, 1, 0.3, 1), (1, 17, 5, 2, 0.1, 1), (2, 24, 4, 1, 0.0, 1), (3, 30, 3, 3, 0.5, 1),
                                            (4, 12, 8, 1, 1.0, 1), (5, 40, 2, 1, 0.05, 1), (7, 33, 64, 0, 0.0, 4), (8, 25, 64, 1, 0.2, 3)]:
        add_graph(f"random seed={seed}", graphgen.make_random_graph(N, M, seed=seed, far_frac=far, groups=groups), fixedp)
    # unusual edge order and range
    add_graph("shuffled", graphgen.make_graph(12, 40, 6, seed=2, shuffle=True), 1)
    ii, jj, kk = chain(300)
    add("targets 200 frames away", ii, np.where(np.arange(jj.size) % 3 == 0, (ii + 200) % 300, jj), kk, 300, 300, 290)
    add("n_all_min and a larger buffer", *chain(20), 64, 512, 2, n_all_min=40)
    # aligned slots (with kernel=k_edge2 also the small ones)
    for drop in (0.0, 0.15, 0.5):
        g = graphgen.make_graph(64, 2048 if drop < 0.3 else 2560, 8, seed=3)
        add(f"ragged 64x2048 drop={drop}", *ragged(g.ii, g.jj, g.kk, drop), g.poses.shape[0], g.patches.shape[0], 1)
        g = graphgen.make_graph(16, 70, 8, seed=5)
        add(f"ragged small drop={drop} repeats", *ragged(g.ii, g.jj, g.kk, drop, repeat=0.2), g.poses.shape[0], g.patches.shape[0], 1)
    add("aligned slots beyond 64", *deep(30, 4, 10, 3), 30, 120, 1)
    # hub tracks
    for n_hubs in (3, 80):
        d, _ = edge_problems.hub_graph(n_hubs)
        add(f"hub_graph({n_hubs})", d["ii"], d["jj"], d["kk"], d["poses"].shape[0], d["patches"].shape[0], 1)
    g = graphgen.make_graph(80, 4, 4, seed=9)
    add("a hub of 70 cameras", *with_track(g.ii, g.jj, g.kk, 41, 10, np.arange(5, 75)), 80, 320, 1)
    for ncam in (32, 33, 65):
        jj = np.arange(1, ncam + 1)
        add(f"one track of {ncam} cameras", np.zeros_like(jj), jj, np.zeros_like(jj), ncam + 1, 4, 1)
    for ncam in (64, 65):
        jj = np.tile(np.arange(1, ncam + 1), 70)
        add(f"70 tracks of {ncam} cameras", np.zeros_like(jj), jj, np.repeat(np.arange(70), ncam), ncam + 1, 128, 1)
    jj = np.tile(np.repeat(np.arange(1, 41), 2), 70)
    add("70 hubs of 40 cameras seen twice", np.zeros_like(jj), jj, np.repeat(np.arange(70), 80), 41, 128, 1)
    # small-tile relayouts
    ii, jj, kk = deep(50, 8, 12, 2)
    add("16-track tiles", ii, jj, kk, 50, 400, 1)
    add("16-track tiles and a loose track", *with_track(ii, jj, kk, 400, 10, np.arange(3, 43)), 50, 408, 1)
    rng = np.random.default_rng(0)
    m, K, n_buf = 3000, 26, 120
    src = rng.integers(0, n_buf - K - 4, m)
    ii = np.repeat(src, K)
    add("many small tiles", ii, ii + np.tile(np.arange(K), m), np.repeat(np.arange(m), K), n_buf, m, 1)
    kk = np.repeat(np.arange(100), 26)
    add("16-track tiles of more than 64 pairs", kk, np.clip(kk + np.tile(np.arange(26), 100), 0, 127), kk, 128, 100, 120)
    kk = np.repeat(np.arange(64), 300)
    add("a (track, pair) seen 300 times", kk // 8, kk // 8 + 1, kk, 10, 64, 1)
    # pair bound and solver size
    rng = np.random.default_rng(3)
    N, M = 100, 3
    kk = np.repeat(np.arange(N * M), 9)
    jj = np.clip(kk // M + rng.integers(-6, 7, kk.size), 0, N - 1)
    for fixedp in (99, 97, 50, 1):
        add(f"mostly fixed trajectory fixedp={fixedp}", kk // M, jj, kk, N, N * M, fixedp)
    for filled in (False, True):
        ii, jj, kk, N, P = edge_problems.band_120(filled)
        add(f"band_120({filled})", ii, jj, kk, N, P, 1)
    for N in (256, 257, 2049, 2050):
        add(f"chain of {N - 1} free poses", *chain(N), N, N, 1)
    # sharding
    rng = np.random.default_rng(17)
    N, M = 40, 5
    kk = np.repeat(np.arange(N * M, dtype=np.int64), rng.integers(1, 9, N * M))
    ii = kk // M
    jj = np.where(rng.random(kk.size) < 0.2, rng.integers(0, N, kk.size), np.clip(ii + rng.integers(-4, 5, kk.size), 0, N - 1))
    for world in (2, 3, 8):
        for r, own in enumerate(partition_tracks(kk, world)):
            add(f"irregular rank {r}/{world}", ii, jj, kk, N, N * M, 2, own=plan_range(own, N * M))
    add("irregular, an empty range", ii, jj, kk, N, N * M, 2, own=plan_range((7, 7), N * M))
    # degenerate lists
    e = np.zeros(0, np.int64)
    add("E = 0", e, e, e, 4, 8, 1)
    for name, (make, fixedp) in edge_problems.CASES.items():
        d = make()
        add(name, d["ii"], d["jj"], d["kk"], d["poses"].shape[0], d["patches"].shape[0], fixedp)
    add("two source frames for a track", [0, 1], [2, 3], [5, 5], 4, 8, 1)
    add("a frame out of range", [0, 1], [2, 9], [5, 6], 4, 8, 1)
    add("a patch out of range", [0, 1], [2, 3], [5, 8], 4, 8, 1)
    # refused arguments and sizes
    add("n_all_min beyond the buffer", [0], [1], [0], 4, 8, 1, n_all_min=5)
    add("a buffer of 40000 frames", [0], [1], [0], 40000, 8, 1)
    add("2^31 patches", e, e, e, 4, 2 ** 31, 1)
    add("a range the wrong way round", [0], [1], [0], 4, 8, 1, own=(5, 3))
    add("a track of 70000 observations", np.zeros(70000), np.ones(70000), np.zeros(70000), 2, 4, 1)
    add("irregular rank 0/2, every pose fixed", ii, jj, kk, N, N * M, N, own=plan_range(partition_tracks(kk, 2)[0], N * M))
    return out


def timing_cases():
    g = graphgen.make_config("C3", seed=0)
    yield "C3", [g.ii, g.jj, g.kk], g.poses.shape[0], g.patches.shape[0], 1, 0, (0, 0)
    g, fp = graphgen.make_window_graph(n_frames=50, M=256, seed=4)
    yield "window 50x256", [g.ii, g.jj, g.kk], g.poses.shape[0], g.patches.shape[0], fp, 0, (0, 0)
    N, M, K = 64, 16384, 8                                    # (the edge list alone: make_graph's inputs are not needed)
    kk = np.repeat(np.arange(N * M, dtype=np.int64), K)
    yield "64x16384x8", [kk // M, np.clip(kk // M + np.tile(np.arange(K, dtype=np.int64) - 3, N * M), 0, N - 1), kk], N, N * M, 1, 0, (0, 0)


if __name__ == "__main__":
    with open(sys.argv[1], "wb") as f:
        for idx, (name, (ii, jj, kk), n_buf, p_tot, fixedp, n_all_min, own) in enumerate(timing_cases() if "--timing" in sys.argv else cases()):
            ii, jj, kk = (np.ascontiguousarray(np.asarray(a, np.int64)) for a in (ii, jj, kk))
            np.array([kk.size, n_buf, p_tot, fixedp, n_all_min, own[0], own[1]], np.int64).tofile(f)
            for a in (ii, jj, kk):
                a.tofile(f)
            print(f"case {idx}: {name}  E={kk.size} n_buf={n_buf} p_tot={p_tot} fixedp={fixedp} own={own}")
