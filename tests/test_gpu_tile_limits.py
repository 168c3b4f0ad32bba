"""-m gpu: the default routes stepped AT the planner's tile-layout limits (ba_plan.cpp; tests/test_plan_cpu.py checks the layouts on the
CPU only): kTileCamF64 = 32 and kTileCamHard = 64 cameras per tile, kFewHubs = 64 loose tracks, kMaxTilePairs = 192 pairs per tile,
64 pairs per pair-major tile, 255 rounds, kSpGroupMax = 32 tiles per group of the pair finalisation.  LDS carve-ups, 8-bit local
indices and group sums go wrong at exactly those values; every case asserts on the uploaded plan that it sits on its boundary (or
one past it), then steps pose+structure and structure-only against oracle.ba_step in float64 under the gates of
tests/test_gpu_jacobian_kernels.py by the plan's edge precision."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import force
import oracle
from batrack_amd import graphgen
from edge_problems import reprojected
from gpu_util import HipProblem, rel, update_err
from test_gpu_jacobian_kernels import GATES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def step_vs_oracle(d, fixedp, label, expect=None):
    """pose+structure and structure-only steps of inputs d against the float64 oracle, GATES by the plan's edge precision
    -> the pose+structure step's outputs (plan, stepper, ...)"""
    ref = oracle.ba_step(d["poses"], d["patches"], d["mono"], d["intrinsics"], d["targets3"], d["weights_pose"], d["ii"], d["jj"], d["kk"],
                         d["bounds"], fixedp=fixedp, want_system=True)
    ref_so = oracle.ba_step(d["poses"], d["patches"], d["mono"], d["intrinsics"], d["targets3"], d["weights"], d["ii"], d["jj"], d["kk"],
                            d["bounds"], fixedp=fixedp, structure_only=True)
    hp = HipProblem(d)
    o = hp.raw_step("weights_pose", fixedp)
    plan = o["plan"]
    if expect is not None:
        expect(plan)
    t_state, t_sys, t_dx, t_upd_p, t_upd_d = GATES[plan.edge_precision]
    act, n = np.unique(d["kk"]), plan.n
    assert o["status"] == 0 and not ref["failed"]
    e = dict(S=rel(np.tril(o["S_lower"]), np.tril(ref["S"])), y=rel(o["y"], ref["y"]), dx=rel(o["dX"].reshape(-1), ref["dX"].reshape(-1)),
             upd_pose=update_err(o["poses_out"], ref["poses_out"], d["poses"], np.arange(fixedp, fixedp + n)),
             upd_disp=update_err(o["patches_out"][:, 2], ref["patches_out"][:, 2], d["patches"][:, 2], act),
             state=max(rel(o["poses_out"], ref["poses_out"]), rel(o["patches_out"], ref["patches_out"])))
    o_so = hp.raw_step("weights", fixedp, True)
    e_so = dict(upd_disp=update_err(o_so["patches_out"][:, 2], ref_so["patches_out"][:, 2], d["patches"][:, 2], act),
                state=rel(o_so["patches_out"], ref_so["patches_out"]))
    gates = dict(S=t_sys, y=t_sys, dx=t_dx, upd_pose=t_upd_p, upd_disp=t_upd_d, state=t_state)
    print(f"{label}: {plan.jacobian_kernel} prec {plan.edge_precision}, {plan.tiles} tiles of <= {plan.max_tile_cams} cameras: "
          + ", ".join(f"{q} {v:.3g} (gate {gates[q]:g})" for q, v in e.items()) + "; structure-only: "
          + ", ".join(f"{q} {v:.3g} (gate {gates[q]:g})" for q, v in e_so.items()))
    for q, v in list(e.items()) + list(e_so.items()):
        assert v < gates[q], (label, q, v, gates[q])
    assert o_so["poses_out"].tobytes() == d["poses"].astype(np.float32).tobytes()
    return o


# ------------------------------------------------------------------ cameras per tile, loose tracks
def hub_problem(c, h):
    """A 70-frame band (4 tracks per frame, each seen by the 3 frames after its own, one fixed pose) and h hub tracks of frame 0, each
    seen by frames 1 .. c -> inputs, the hubs' patches"""
    g = graphgen.make_graph(87, 4, 3, seed=21)                  # (frames and patches; of its 348 patches the last 68 serve as hubs)
    kk = np.repeat(np.arange(280, dtype=np.int64), 3)
    ii = kk // 4
    jj = ii + np.tile(np.arange(1, 4, dtype=np.int64), 280)
    keep = jj < 70
    hubs = np.arange(280, 280 + h, dtype=np.int64)
    hk = np.repeat(hubs, c)
    ii, jj, kk = (np.concatenate(a) for a in ((ii[keep], np.zeros_like(hk)), (jj[keep], np.tile(np.arange(1, c + 1, dtype=np.int64), h)), (kk[keep], hk)))
    d = reprojected(g, ii, jj, kk, np.random.default_rng(5))
    d.update(poses=d["poses"][:70], intrinsics=d["intrinsics"][:70], patches=d["patches"][:280 + h], mono=d["mono"][:280 + h])
    return d, hubs


HUBS = {(32, 3): dict(loose=0, cams=32, prec=8), (33, 3): dict(loose=3, cams=16, prec=8), (33, 64): dict(loose=64, cams=16, prec=8),
        (33, 65): dict(loose=0, cams=33, prec=8), (64, 65): dict(loose=0, cams=64, prec=4), (65, 65): dict(loose=65, cams=16, prec=8)}


@pytest.mark.skipif(bool(force.tokens()), reason="the default routes are what the test is about")
@pytest.mark.parametrize("c,h", list(HUBS))
def test_hub_tracks_at_the_camera_limits_of_a_tile(c, h):
    """kTileCamF64 = 32: a track of 32 free cameras stays in a tile whose E is float64; of 33, it is LOOSE while the plan has at most
    kFewHubs = 64 such tracks; 65 of them go back into tiles of up to kTileCamHard = 64 cameras (384 rows of E, float32 per edge);
    65 cameras fit no tile.  (The precision is the route's, from the LDS the largest tile takes as double — tile_lds_bytes_r, ba_step.cpp:
    the 33-camera tiles of this list, 208 rows of E and 33 pairs, still fit, so that plan stays float64 per edge and holds those gates.)"""
    d, hubs = hub_problem(c, h)
    want = HUBS[(c, h)]

    def expect(plan):
        loc, kx = plan.array("trk_loc"), plan.array("kx")
        assert sorted(kx[loc < 0]) == (sorted(hubs) if want["loose"] else []), (c, h)
        assert int((loc < 0).sum()) == want["loose"]
        assert plan.max_tile_cams == want["cams"] and int(plan.array("tile_ncam").max()) == want["cams"]
        assert plan.edge_precision == want["prec"] and plan.jacobian_kernel == "k_tile"

    step_vs_oracle(d, 1, f"hubs c={c} h={h}", expect)


# ------------------------------------------------------------------ pairs per tile
@pytest.mark.skipif(bool(force.tokens()), reason="the default routes are what the test is about")
@pytest.mark.parametrize("fixedp", [99, 97, 90, 50])
def test_a_tile_with_192_pairs(fixedp):
    """The mostly-fixed trajectory of tests/test_plan_cpu.py: 64 tracks fill a tile long before its camera budget, and the planner closes
    the tile on kMaxTilePairs = 192 pairs — the pair geometry table of a tile, full, with 1, 3, 10 and 16 free cameras in a tile."""
    rng = np.random.default_rng(3)
    N, M = 100, 3
    kk = np.repeat(np.arange(N * M, dtype=np.int64), 9)
    ii = kk // M
    jj = np.clip(ii + rng.integers(-6, 7, kk.size), 0, N - 1).astype(np.int64)
    g = graphgen.make_graph(N, M, 1, seed=8)
    d = reprojected(g, ii, jj, kk, np.random.default_rng(9))

    def expect(plan):
        assert int(plan.array("tile_npair").max()) == 192 and plan.n == N - fixedp

    step_vs_oracle(d, fixedp, f"192 pairs, fixedp {fixedp}", expect)


# ------------------------------------------------------------------ the pair-major layout: pairs per tile, rounds
ETILE = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import test_gpu_tile_limits as tl
case = sys.argv[1]
d, fixedp = tl.etile_case(case)
figures = tl.ETILE_FIGURES[case]

def expect(plan):
    rec = plan.array("pm_rec").reshape(-1, 4)
    got = dict(kernel=plan.jacobian_kernel, tiles=plan.tiles, npair=int(plan.array("tile_npair").max()), pm=int(rec.shape[0]),
               rounds=int((rec[:, 1] >> 8).max()) if rec.size else 0)
    print("ETILE", case, got)
    assert got == figures, (case, got, figures)

tl.step_vs_oracle(d, fixedp, "k_etile forced, " + case, expect)
print("ETILE_OK")
"""


def etile_case(case):
    """-> inputs, fixedp"""
    if case in ("pairs64", "pairs65"):
        # tracks of 16 / 13 FIXED source frames with 4 / 5 free targets each: 64 / 65 pairs in one tile
        nsrc, ntgt = (16, 4) if case == "pairs64" else (13, 5)
        kk = np.repeat(np.arange(nsrc, dtype=np.int64), ntgt)
        jj = nsrc + np.tile(np.arange(ntgt, dtype=np.int64), nsrc)
        g = graphgen.make_graph(nsrc + ntgt, 1, 1, seed=4)
        return reprojected(g, kk.copy(), jj, kk, np.random.default_rng(2)), nsrc
    # one (track, pair) observed 255 / 256 times
    reps = 255 if case == "rounds255" else 256
    g = graphgen.make_graph(2, 1, 1, seed=4)
    return reprojected(g, np.zeros(reps, np.int64), np.ones(reps, np.int64), np.zeros(reps, np.int64), np.random.default_rng(2)), 1


ETILE_FIGURES = {"pairs64": dict(kernel="k_etile", tiles=1, npair=64, pm=1, rounds=1),
                 "pairs65": dict(kernel="k_tile", tiles=1, npair=65, pm=0, rounds=0),
                 "rounds255": dict(kernel="k_etile", tiles=1, npair=1, pm=1, rounds=255),
                 "rounds256": dict(kernel="k_tile", tiles=1, npair=1, pm=0, rounds=0)}


@pytest.mark.parametrize("case", list(ETILE_FIGURES))
def test_pair_major_tiles_at_their_limits(case):
    """Under BT_FORCE kernel=k_etile (read once per process: a child): a tile of 64 pairs and a (track, pair) observed 255 times take the
    pair-major kernel (one lane per pair; 8-bit round counts); 65 pairs and 256 rounds drop the pair-major tables and the plan falls
    back to k_tile — each against the oracle."""
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + ETILE, case],
                       cwd=ROOT, env=force.env_with("kernel=k_etile"), capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "ETILE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ------------------------------------------------------------------ tiles per group of the pair finalisation
@functools.lru_cache(maxsize=None)
def window(M):
    g, fixedp = graphgen.make_window_graph(n_frames=12, M=M, seed=4)
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    return dict(poses=f(g.poses), patches=f(g.patches), mono=f(g.mono_disp), intrinsics=f(g.intrinsics), targets3=f(g.targets3),
                weights=f(g.weights), weights_pose=f(g.weights_pose), ii=g.ii, jj=g.jj, kk=g.kk, bounds=np.asarray(g.bounds, np.float64)), fixedp


@pytest.mark.skipif(bool(force.tokens()), reason="the default routes are what the test is about")
@pytest.mark.parametrize("M,groups", [(528, [32] * 6 + [6]), (512, [32] * 6)])
def test_tile_groups_of_the_pair_finalisation(M, groups):
    """kSpGroupMax = 32: the tiles of one camera set are summed in groups of at most 32 (k_pair_finalize).  A window of 12 frames with
    528 patches per frame has 33 tiles per keyframe: full groups and a remainder of 6; with 512, groups of exactly 32."""
    d, fixedp = window(M)

    def expect(plan):
        assert np.diff(plan.array("sg_ptr")).tolist() == groups and int(plan.array("tile_ntrk").max()) == 16

    step_vs_oracle(d, fixedp, f"window 12 x {M}", expect)
