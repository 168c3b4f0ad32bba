"""The graphs of tests/wpt_graphs.py through the host planner, without a GPU: every graph has the layout it is named for under
either forced wave-per-tile kernel, and under every launch cap of tests/test_gpu_wpt_walks.py (BT_FORCE wptwaves=N) the tile
ranges the launchers form reach the code that carries state from tile to tile.  A planner change that silently moved a graph off
its path fails here, not nowhere.

BT_FORCE is read once per process: one child process per forced kernel lays out all graphs (upload=False) and prints the tables
the checks need; the tests compare them with the figures below.

What "reaches" means is read off the kernels (ba_edge2.hip, ba_edge2u.hip, ba_stream.hip): a wave (k_stream: a workgroup) walks the
tiles [w tpw, (w + 1) tpw) with tpw = ceil(T / max_waves); its first tile counts as new cameras and a new pair list whatever the
flags; k_edge2 keeps a lane's pair sums while `same_slots` holds (flags & 2, the same lgS, the same (local pair, repeat, used) in
every slot) and sends them off after kPaFlushTiles = 16 tiles; at the end the waves of a k_edge2 workgroup are merged pairwise
(wave w with w + stride, stride 1, 2) where their row counts and global rows, or slot counts and global pairs, agree."""
import collections
import functools
import json
import os
import subprocess
import sys

import pytest

import wpt_graphs as wg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1])
import wpt_graphs as wg
from batrack_amd.plan import Plan
out = {}
for name in wg.GRAPHS[sys.argv[2]]:
    ii, jj, kk, n_buf, p_tot, fixedp = wg.edges(name)
    pl = Plan(ii, jj, kk, n_buf, p_tot, fixedp, upload=False)
    A = pl.arrays()
    t = wg.tile_table(A)
    T = pl.tiles
    cam0, pair0 = A["tile_cam0"], A["tile_pair0"]
    g = dict(tiles=T, max_tile_cams=pl.max_tile_cams, n=pl.n, it_edge=int(A["it_edge"].size), E=int(kk.size),
             flags=t["flags"].tolist(), lgS=None if A["it_edge"].size == 0 else t["lgS"].tolist(),
             **{k: t[k].tolist() for k in ("ntrk", "ncam", "npair", "nslot")},
             cams=[A["tile_cams"][cam0[i]:cam0[i] + t["ncam"][i]].tolist() for i in range(T)],
             pairs=[A["tile_pairs"][pair0[i]:pair0[i] + t["npair"][i]].tolist() for i in range(T)])
    if A["it_edge"].size:
        # what each of the 64 lanes of k_edge2 holds of tile_sinfo (slot = lane & (S - 1)): the bits same_slots compares
        si = A["tile_sinfo"].reshape(T, 64)
        lane = np.arange(64)
        g["sig"] = [(si[i, lane & ((1 << t["lgS"][i]) - 1)] & 0x2ff00).tolist() for i in range(T)]
    out[name] = g
print("WPT_JSON " + json.dumps(out))
"""


@functools.lru_cache(maxsize=None)
def plans(kernel):
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, kernel], cwd=ROOT, env=dict(os.environ, BT_FORCE=f"kernel={kernel}", PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("WPT_JSON ")][-1]
    return json.loads(line[len("WPT_JSON "):])


def hist(v):
    return dict(sorted(collections.Counter(v).items()))


# ------------------------------------------------------------------ the layouts
# tiles, histogram of flags & 3 (1: the cameras of the tile before, 3: its pair list too), the lgS of the edge-major records (None: no
# edge-major tables — some tile has more than 64 slots), the largest slot count, max_tile_cams, the track counts that occur
E2 = {
    "band":     (48, {0: 12, 3: 36}, {2, 3}, 8, 9, {8, 64}),
    "ragged":   (48, {0: 12, 3: 36}, {2, 3}, 8, 9, {6, 7, 8, 64}),
    "repeats":  (48, {0: 12, 3: 36}, {4, 5, 6}, 40, 9, {8, 64}),
    "selfe":    (48, {0: 12, 3: 36}, {3}, 5, 5, {8, 64}),
    "oneframe": (21, {0: 1, 3: 20}, {2}, 4, 3, {5, 64}),
    "cams9":    (42, {0: 14, 3: 28}, {0, 1, 2, 3, 4}, 9, 10, {2, 64}),
    "cams10":   (42, {0: 14, 3: 28}, {0, 1, 2, 3, 4}, 10, 11, {2, 64}),
    "cams11":   (42, {0: 14, 3: 28}, {0, 1, 2, 3, 4}, 11, 12, {2, 64}),
    "slots1":   (25, {0: 4, 1: 1, 3: 20}, {0}, 1, 2, {4, 64}),
    "slots2":   (25, {0: 5, 3: 20}, {0, 1}, 2, 3, {4, 64}),
    "slots3":   (25, {0: 4, 1: 1, 3: 20}, {0, 1, 2}, 3, 3, {4, 64}),
    "slots5":   (25, {0: 2, 1: 3, 3: 20}, {0, 1, 2, 3}, 5, 3, {4, 64}),
    "deep":     (13, {0: 9, 1: 3, 3: 1}, None, 68, 6, {32, 64}),
    "fewcams":  (6, {0: 1, 1: 2, 3: 3}, {6}, 44, 1, {32, 64}),
}
# under k_stream the tiles run across source frames (64 tracks each): also the largest pair list
ST = {
    "band":     (38, {0: 13, 1: 9, 3: 16}, None, 8, 10, {32, 64}, 16),
    "ragged":   (38, {0: 13, 1: 9, 3: 16}, None, 8, 10, {29, 64}, 16),
    "repeats":  (38, {0: 13, 1: 9, 3: 16}, None, 16, 10, {32, 64}, 16),
    "selfe":    (38, {0: 16, 1: 6, 3: 16}, None, 5, 6, {32, 64}, 10),
    "oneframe": (21, {0: 1, 3: 20}, None, 4, 3, {5, 64}, 4),
    "cams9":    (29, {0: 16, 1: 11, 3: 2}, None, 9, 11, {28, 64}, 18),
    "cams10":   (29, {0: 15, 1: 12, 3: 2}, None, 10, 12, {28, 64}, 20),
    "cams11":   (29, {0: 14, 1: 13, 3: 2}, None, 11, 12, {28, 64}, 22),
    "slots1":   (21, {0: 5, 1: 4, 3: 12}, None, 1, 3, {20, 64}, 2),
    "slots2":   (21, {0: 5, 1: 4, 3: 12}, None, 2, 3, {20, 64}, 4),
    "slots3":   (21, {0: 4, 1: 5, 3: 12}, None, 3, 3, {20, 64}, 6),
    "slots5":   (21, {0: 2, 1: 7, 3: 12}, None, 5, 3, {20, 64}, 9),
    "deep":     (13, {0: 9, 1: 3, 3: 1}, None, 68, 6, {32, 64}, 8),
}
FIGURES = {"k_edge2": E2, "k_stream": ST}
CASES = [(k, n) for k in ("k_edge2", "k_stream") for n in wg.GRAPHS[k]]


def route(kernel, g):
    """the Jacobian kernel plan_route (ba_step.cpp) gives the plan under BT_FORCE kernel=`kernel`: k_edge2 where the edge-major tables
    exist, k_stream for tiles of at most 32 pairs — both for tiles of at most 10 cameras —, else k_tile"""
    small = 0 < g["max_tile_cams"] <= 10
    if kernel == "k_edge2" and g["it_edge"] and small and max(g["npair"]) <= 64:
        return "k_edge2"
    return "k_stream" if small and max(g["npair"]) <= 32 else "k_tile"


# the kernel every graph must take on the device (tests/test_gpu_wpt_walks.py asserts it of the uploaded plan): the forced one, but
# for the fall-through cases — tiles of 11 and more cameras, tiles of more than 64 slots
KERNEL = {"k_edge2": dict({n: "k_edge2" for n in wg.GRAPHS["k_edge2"]}, cams10="k_tile", cams11="k_tile", deep="k_stream"),
          "k_stream": dict({n: "k_stream" for n in wg.GRAPHS["k_stream"]}, cams9="k_tile", cams10="k_tile", cams11="k_tile")}


@pytest.mark.parametrize("kernel,name", CASES)
def test_every_graph_has_the_layout_it_is_named_for(kernel, name):
    g = plans(kernel)[name]
    want = FIGURES[kernel][name]
    got = (g["tiles"], hist(g["flags"]), None if g["lgS"] is None else set(g["lgS"]), max(g["nslot"]), g["max_tile_cams"], set(g["ntrk"]))
    assert got == want[:6], (kernel, name, got)
    assert (g["it_edge"] > 0) == (want[2] is not None)
    assert max(g["ncam"]) == g["max_tile_cams"]
    if kernel == "k_stream":
        assert max(g["npair"]) == want[6]
    assert route(kernel, g) == KERNEL[kernel][name]
    assert g["E"] <= 44200


def test_the_named_shapes():
    e2, st = plans("k_edge2"), plans("k_stream")
    # oneframe: 20 full tiles and one of 5 tracks, one pair list; 21 tiles under k_stream as well
    assert e2["oneframe"]["ntrk"] == [64] * 20 + [5] and e2["oneframe"]["flags"] == [0] + [3] * 20 and st["oneframe"]["flags"] == [0] + [3] * 20
    # band: four tiles per source frame under k_edge2, the first with new cameras
    assert e2["band"]["flags"] == [0, 3, 3, 3] * 12 and e2["band"]["ntrk"] == [64, 64, 64, 8] * 12
    # repeats under k_stream: an odd slot count (the chunk split of the two waves), more than one slot group; slots K: 1 slot
    assert any(s % 2 for s in st["repeats"]["nslot"]) and set(st["slots1"]["nslot"]) == {1}
    # deep: 68 slots in some tile — more than the edge-major layout holds, so the forced k_edge2 falls to k_stream
    assert max(e2["deep"]["nslot"]) == 68 and e2["deep"]["it_edge"] == 0
    # slots K: the lgS of consecutive tiles differ inside the list (LGS = -1 instantiations)
    for name, lgs in (("slots2", [1, 0]), ("slots3", [2, 1, 0]), ("slots5", [3, 2, 1, 0])):
        seq = e2[name]["lgS"]
        assert [a for a, b in zip(seq, seq[1:] + [-1]) if a != b] == lgs, (name, seq)
    # k_stream: all three kinds of flags in slots K and band: new cameras, the same cameras with another pair list, both the same
    for name in ("band", "slots1", "slots2", "slots3", "slots5"):
        assert set(st[name]["flags"]) == {0, 1, 3}, name
    # fewcams: 12 + 12 observations in 44 aligned slots per track (S = 64) and ONE free camera: the pair sums of the S slots do not
    # fit the dead local E at the end of k_edge2 (`pcomb`, ba_edge2.hip: S 26 doubles against 6 max_cams rows of e_row(0) = 68 floats)
    f = e2["fewcams"]
    S = 1 << max(f["lgS"])
    assert S == 64 and f["max_tile_cams"] == 1 and S * 26 * 8 > 6 * f["max_tile_cams"] * 68 * 4 and S <= 2 * 64
    for name in wg.GRAPHS["k_edge2"]:                         # ... and every other k_edge2 graph does fit (the `pcomb` branch)
        g = e2[name]
        if name != "fewcams" and KERNEL["k_edge2"][name] == "k_edge2":
            row = 20 if set(g["lgS"]) == {3} and g["max_tile_cams"] <= 8 else 68
            assert (1 << max(g["lgS"])) * 26 * 8 <= 6 * g["max_tile_cams"] * row * 4 and (1 << max(g["lgS"])) <= 2 * (row - 4), name


# ------------------------------------------------------------------ the launches under every cap
def e2_waves_per_workgroup(g, lmbda_trk=False):
    """e2::launch_t: waves per workgroup = min(4, LDS of a CU (160 KB on gfx950) / one wave's slice (lds_bytes))"""
    mtp, mc = max(max(g["npair"]), 1), g["max_tile_cams"]
    lgs = 3 if set(g["lgS"]) == {3} and mc <= 8 else -1
    row = {3: 16}.get(lgs, 64) + 4
    nt = 3 if mc <= 8 else 4
    rmax = 6 * mc
    b = (128 + 4 + 64 + nt * (nt + 1) // 2 * 256 + mtp * 18) * 8 + (128 + 2 * (row - 4) + rmax * row + ((rmax + 3) & ~3) + mtp * 20 + (64 if lmbda_trk else 0)) * 4
    b = (b + 255) & ~255
    return min(4, 8, 160 * 1024 // b)


def walk_e2(g, b, e):
    """k_edge2's pair-sum bookkeeping over the tiles [b, e) of one wave -> (flushes after kPaFlushTiles tiles that are followed by more
    tiles of the same slots, tiles with flags & 2 and the same lgS whose slot signature differs from the tile before)"""
    pa_tiles, pa_lgS, full, sig_only = 0, 0, 0, 0
    for t in range(b, e):
        fl = 0 if t == b else g["flags"][t]
        same_sig = t > b and g["sig"][t] == g["sig"][t - 1]
        same = bool(fl & 2) and g["lgS"][t] == pa_lgS and same_sig
        if (fl & 2) and g["lgS"][t] == pa_lgS and not same_sig:
            sig_only += 1
        if same and pa_tiles >= 16:
            full += 1
        if not same or pa_tiles >= 16:
            pa_tiles = 0
        if not same:
            pa_lgS = g["lgS"][t]
        pa_tiles += 1
    return full, sig_only


def reached(kernel, name, cap):
    g = plans(kernel)[name]
    T = g["tiles"]
    r = dict(longest=0, cam_change=0, pair_change=0, kept=0, idle=0, full=0, sig_only=0, lgs_change=0, tree_rows=0, tree_pairs=0)
    rng = wg.ranges(T, cap)
    for b, e in rng:
        run = 1
        for t in range(b + 1, e):
            fl = g["flags"][t]
            run = run + 1 if fl & 2 else 1
            r["longest"] = max(r["longest"], run)
            r["cam_change"] += (not fl & 1) and t + 1 < e          # new cameras in the middle of a range, and the range goes on
            r["pair_change"] += (fl & 3) == 1 and t + 1 < e        # the same cameras with a new pair list
            r["kept"] += (fl & 3) == 3                             # sums kept in registers / LDS from one tile to the next
            if g["lgS"] is not None:
                r["lgs_change"] += g["lgS"][t] != g["lgS"][t - 1]
        if kernel == "k_edge2":
            full, sig_only = walk_e2(g, b, e)
            r["full"] += full; r["sig_only"] += sig_only
    if kernel == "k_edge2":
        W = e2_waves_per_workgroup(g)
        tpw, nw, nb = wg.launch(T, cap, W)
        r["idle"] = W * nb - nw
        # the end-of-kernel tree: wave wv of workgroup blk walks range nb W - 1 - (blk W + wv) (the launch's first waves take the last tiles)
        for blk in range(nb):
            held = {}
            for wv in range(W):
                gwt = nb * W - 1 - (blk * W + wv)
                if gwt < nw:
                    last = rng[gwt][1] - 1
                    held[wv] = (6 * g["ncam"][last], g["cams"][last], g["lgS"][last], [p if s & 0x20000 else -1 for p, s in zip(_lane_pairs(g, last), g["sig"][last])])
            for stride in (1, 2):
                for wv in range(0, W, 2 * stride):
                    if wv in held and wv + stride in held:
                        a, c = held[wv], held[wv + stride]
                        r["tree_rows"] += a[0] == c[0] and a[1] != c[1]        # as many rows, other cameras: must not be merged
                        r["tree_pairs"] += a[2] == c[2] and a[3] != c[3]       # as many slots, other pairs
    return r


def _lane_pairs(g, t):
    """global pair of every lane's slot in tile t (pa_gp)"""
    return [g["pairs"][t][min((g["sig"][t][ln] >> 8) & 0xff, len(g["pairs"][t]) - 1)] for ln in range(64)]


def test_one_wave_walks_seventeen_tiles_of_one_pair_list():
    for kernel in ("k_edge2", "k_stream"):
        assert wg.launch(21, 1, 1)[:2] == (21, 1)
        r = reached(kernel, "oneframe", 1)
        assert r["longest"] >= 17 and r["kept"] == 20, (kernel, r)
    assert reached("k_edge2", "oneframe", 1)["full"] == 1          # flush_pairs() on pa_tiles >= kPaFlushTiles, once, four tiles before the end
    assert all(reached(k, "oneframe", None)["longest"] == 0 for k in ("k_edge2", "k_stream"))     # uncapped: a tile per wave


@pytest.mark.parametrize("kernel", ["k_edge2", "k_stream"])
def test_ranges_cross_camera_changes_and_go_on(kernel):
    """new cameras in the middle of a wave's range with tiles behind them (flush_schur and the rewrite of gidx; k_stream: new_cams and the
    barrier), next to tiles that keep the sums of the tile before — at every cap on the band graphs, at caps 1 and 3 on the small ones"""
    banded = ("band", "ragged", "repeats", "selfe")
    for name in banded + ("slots2", "slots3", "slots5") + (("deep",) if kernel == "k_stream" else ("cams9",)):
        for cap in (1, 3, 7) if name in banded else (1, 3):
            r = reached(kernel, name, cap)
            assert r["cam_change"] >= 1 and r["kept"] >= 1, (kernel, name, cap, r)
        r = reached(kernel, name, None)                        # without a cap: a tile per wave, nothing carried
        assert r["cam_change"] == r["pair_change"] == r["kept"] == r["longest"] == 0, (kernel, name, r)
    # the same cameras under a new pair list in the middle of a range (k_stream: new_pairs without new_cams; k_edge2 / k_edge2u: the
    # geometry reload on !(flags & 2) without a flush of the Schur sums)
    for name in ("band", "ragged", "repeats", "selfe", "slots1", "slots2", "slots3", "slots5", "deep") if kernel == "k_stream" else ("slots5", "fewcams"):
        assert reached(kernel, name, 1)["pair_change"] >= 1, (kernel, name)
    if kernel == "k_stream":
        assert all(reached(kernel, "band", cap)["pair_change"] >= 8 for cap in (1, 3, 7))


def test_edge2_paths_under_the_caps():
    # a workgroup holds a wave without tiles at every cap (W nb > nw), also without a cap where the tiles do not fill the last one
    for name in wg.GRAPHS["k_edge2"]:
        if KERNEL["k_edge2"][name] != "k_edge2":
            continue
        for cap in (1, 3, 7):
            g = plans("k_edge2")[name]
            W = e2_waves_per_workgroup(g)
            tpw, nw, nb = wg.launch(g["tiles"], cap, W)
            assert nw <= cap and (tpw > 1 or g["tiles"] <= cap)
        assert reached("k_edge2", name, 1)["idle"] >= 1, name
    # (workgroups of four waves, of three where the tiles see ten cameras: both shapes of the end-of-kernel tree)
    assert e2_waves_per_workgroup(plans("k_edge2")["cams9"]) == 3 and e2_waves_per_workgroup(plans("k_edge2")["band"]) == 4
    # lgS changes from tile to tile inside a range (LGS = -1: the local E is cleared, the lane groups change)
    for name in ("band", "repeats", "cams9", "slots2", "slots3", "slots5"):
        assert all(reached("k_edge2", name, cap)["lgs_change"] >= 1 for cap in (1, 3)), name
    # flags & 2 and the same lgS, but another (pair, repeat, used) in some slot: the tile_sinfo comparison of same_slots decides alone
    assert all(reached("k_edge2", "repeats", cap)["sig_only"] >= 1 for cap in (1, 3, 7))
    # partners of the end-of-kernel tree with as many rows but other cameras, with as many slots but other pairs
    for name in ("band", "ragged", "repeats", "selfe", "cams9"):
        r = reached("k_edge2", name, 7)
        assert r["tree_rows"] >= 1, (name, r)
    assert all(reached("k_edge2", name, 7)["tree_pairs"] >= 1 for name in ("band", "ragged", "repeats", "selfe"))
