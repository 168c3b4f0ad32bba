"""The construction of tests/mask_problems.py against the oracle, without a GPU: every tagged edge is on the side of its threshold
the tag says, in float64 AND in float32; no edge, tagged or not, is closer to a threshold than the margins (so that a kernel that
differs from the oracle by rounding cannot flip a decision, and one that flips a decision is wrong); the clamp tracks end on
their bound exactly; the systems are as well conditioned as the fixtures'; and the planner's tables, stepped by the emulator on
the base problem, give the oracle's result."""
import numpy as np
import pytest

import oracle
import mask_problems as mp
from batrack_amd.plan import Plan
from plan_emulator import run as emulate

EDGE_TAGS = ["z_zero", "z_thin", "z_behind", "z_behind_axis", "z_mixed", "out_l", "out_r", "out_t", "out_b", "in_l", "in_r", "in_t", "in_b",
             "r_249", "r_251", "knee", "clamp_lo", "clamp_hi"]
TRACK_TAGS = EDGE_TAGS + ["z_thin_dj", "z_thin_iz", "start_out_hi", "start_out_lo", "all_masked_track"]
B = mp.BOUNDS


def rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / max(np.linalg.norm(b), 1e-300)


def ulps(x, n=1000):
    return n * np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def edges(name, dtype, loss="huber"):
    d = mp.problem(name)[0]
    return oracle.edges(d["poses"], d["patches"], d["intrinsics"], d["targets3"], d["weights_pose"], d["ii"], d["jj"], d["kk"], d["bounds"],
                        loss=loss, dtype=dtype)


def raw_residual(d, e):
    return d["targets3"][:, :2] - np.asarray(e["coords"], np.float64)        # (e["r"] is masked)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_tag_is_present_and_valid_as_the_table_says(dtype):
    d, info = mp.problem("base")
    e = edges("base", dtype)
    assert all(np.isfinite(v).all() for v in e.values())                    # nothing non-finite, the point on a camera's plane included
    for tag in EDGE_TAGS:
        ed, valid = info["edge_tags"][tag]
        assert len(ed) > 0 and np.array_equal(e["valid"][ed], valid), (tag, e["valid"][ed], valid)
    for tag in TRACK_TAGS:
        assert info["track_tags"].get(tag), tag
        assert all(p in info["special"] for p in info["track_tags"][tag])
    Z, tr = mp.edge_z(d), info["track_tags"]
    of = lambda tag: np.flatnonzero(np.isin(d["kk"], tr[tag]))
    # z_zero: on the plane of camera 1; zero Jacobians there
    (e0,), _ = info["edge_tags"]["z_zero"]
    assert d["jj"][e0] == 1 and abs(Z[e0]) < 1e-6 and not e["Jj"][e0].any() and not e["Ji"][e0].any() and not e["Jz"][e0].any()
    # z_thin: dj = 0 with Z between the reprojection's clamp and 0.2; and Z under the clamp
    assert any(2e-2 <= z <= 0.15 for z in Z[of("z_thin_dj")]) and any(0 < z <= 5e-3 for z in Z[of("z_thin_iz")])
    for tag in ("z_thin_dj", "z_thin_iz"):
        thin = of(tag)[np.abs(Z[of(tag)]) < 0.2]
        assert len(thin) and not e["Jj"][thin].any()
    # z_behind: well behind at least two cameras, where dj != 0 and only vld masks
    eb, _ = info["edge_tags"]["z_behind"]
    assert len(eb) >= 2 and (Z[eb] < -0.5).all() and all(e["Jj"][x].any() for x in eb)
    # ... and behind a camera on its axis: Z > 0.2 is the one comparison that fails
    (ea,), _ = info["edge_tags"]["z_behind_axis"]
    ua, va = e["coords"][ea]
    assert Z[ea] < -0.25 and mp.inside(ua, va) and mp.uv_clear(ua, va, 100.0) and np.linalg.norm(raw_residual(d, e)[ea]) < 5 and e["Jj"][ea].any()
    # z_mixed: two valid and two masked edges in one track
    em, vm = info["edge_tags"]["z_mixed"]
    assert len(set(d["kk"][em])) == 1 and sorted(vm) == [0, 0, 1, 1] and (Z[em[vm == 0]] < 0.2).all() and (Z[em[vm == 1]] > 0.2).all()
    # all_masked_track: no valid edge
    for p in tr["all_masked_track"]:
        assert not e["valid"][d["kk"] == p].any()
    # out_*: only the one comparison fails, and the track keeps a valid edge; in_*: within 8 px inside
    u, v = np.asarray(e["coords"], np.float64).T
    r = np.linalg.norm(raw_residual(d, e), axis=1)
    for s, (gone, dist) in {"l": (u <= B[0], u - B[0]), "r": (u >= B[2], B[2] - u), "t": (v <= B[1], v - B[1]), "b": (v >= B[3], B[3] - v)}.items():
        ed, _ = info["edge_tags"]["out_" + s]
        fails = (u <= B[0]).astype(int) + (u >= B[2]) + (v <= B[1]) + (v >= B[3])
        assert gone[ed].all() and (fails[ed] == 1).all() and (Z[ed] > 0.25).all() and (r[ed] < 249).all(), s
        assert e["valid"][of("out_" + s)].any()
        (x, y, _), = d["patches"][tr["out_" + s]]
        assert {"l": x - B[0], "r": B[2] - x, "t": y - B[1], "b": B[3] - y}[s] == 3.0
        ed, _ = info["edge_tags"]["in_" + s]
        assert ((dist[ed] > 0) & (dist[ed] <= 8.0)).all(), s
    # |r| on either side of 250, along an axis and along the diagonal
    for tag, lo, hi in (("r_249", 248.5, 249.5), ("r_251", 250.5, 252.5)):
        ed, _ = info["edge_tags"][tag]
        assert ((r[ed] > lo) & (r[ed] < hi)).all() and (Z[ed] > 0.25).all() and all(mp.inside(a, b) for a, b in zip(u[ed], v[ed])), tag
        rr = np.abs(raw_residual(d, e)[ed])
        assert (rr[:, 1] < 1e-3).any() and (np.abs(rr[:, 0] - rr[:, 1]) < 1e-3).any()
    # the knee: 0.9 and 1.1 with both signs on both components; huber weight 1 and 1 / |r|
    ed, _ = info["edge_tags"]["knee"]
    rk = raw_residual(d, e)[ed]
    for c in (0, 1):
        assert sorted(np.round(rk[:, c], 2)) == [-1.1, -0.9, 0.9, 1.1]
    rho = e["W"][ed] / d["weights_pose"][ed]
    assert np.allclose(rho, np.where(np.abs(rk) > 1, 1 / np.abs(rk), 1.0), rtol=1e-4, atol=0)


@pytest.mark.parametrize("name", ["base", "deep", "loose"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_no_edge_is_near_a_threshold(name, dtype):
    """Margins of at least 1000 float32 ulps of the quantity compared, on every edge, tagged or not."""
    d, info = mp.problem(name)
    e = edges(name, dtype)
    Z = mp.edge_z(d)
    on_plane = np.zeros(len(Z), bool)
    if "z_zero" in info["edge_tags"]:
        on_plane[info["edge_tags"]["z_zero"][0]] = True
        assert (np.abs(Z[on_plane]) < 1e-6).all()
    gap02 = np.abs(np.abs(Z) - 0.2)
    assert (gap02 >= mp.M_Z02 - 1e-12).all() and (gap02 >= ulps(0.2)).all(), gap02.min()
    assert ((Z >= 2e-2) | (Z <= 5e-3)).all()                                     # a factor of 2 from the reprojection's clamp
    u, v = np.asarray(e["coords"], np.float64).T
    for x, lo, hi in ((u, B[0], B[2]), (v, B[1], B[3])):
        gap = np.minimum(np.abs(x - lo), np.abs(x - hi))
        assert (gap >= mp.M_UV).all() and (gap >= ulps(x)).all(), gap.min()
    rr = raw_residual(d, e)
    r = np.linalg.norm(rr, axis=1)
    assert (np.abs(r - 250.0) >= mp.M_R).all() and (np.abs(r - 250.0) >= ulps(r)).all(), np.abs(r - 250.0).min()
    # the huber knee, per component (edges in front of their camera: elsewhere the weight is masked whatever it is)
    front = Z > 0.2
    assert (np.abs(np.abs(rr[front]) - 1.0) >= mp.M_KNEE).all(), np.abs(np.abs(rr[front]) - 1.0).min()
    # both precisions decide alike, and as the tags say
    assert np.array_equal(e["valid"], edges(name, np.float64)["valid"])
    for tag in ("hub_z_mixed", "hub_out", "hub_in", "clamp_hi") if name == "loose" else EDGE_TAGS:
        ed, valid = info["edge_tags"][tag]
        assert len(ed) > 0 and np.array_equal(e["valid"][ed], valid), tag
    if name == "loose":
        assert set(info["edge_tags"]["hub_z_mixed"][1]) == {0.0, 1.0} and (Z[info["edge_tags"]["hub_z_mixed"][0]] < -0.5).sum() >= 20
        u_o, v_o = (x[info["edge_tags"]["hub_out"][0]] for x in (u, v))
        assert ((u_o > B[2]) & (v_o > B[1])).any() and (v_o < B[1]).any()            # through the right border alone, and through the top


@pytest.mark.parametrize("name", ["base", "deep", "loose"])
def test_masked_share_and_conditioning(name):
    d, info = mp.problem(name)
    valid = edges(name, np.float64)["valid"] > 0
    assert 0 < (~valid).sum() <= len(valid) / 4, (~valid).sum()
    n_all = int(max(d["ii"].max(), d["jj"].max())) + 1
    for pose in range(info["fixedp"], n_all):
        assert (valid & ((d["ii"] == pose) | (d["jj"] == pose))).sum() >= 20, pose
    for case, (prob, so, loss) in mp.CASES.items():
        if prob != name or so:
            continue
        r64, r32 = mp.reference(case), mp.reference(case, np.float32)
        assert not r64["failed"] and not r32["failed"]
        assert all(np.isfinite(r64[k]).all() for k in ("S", "y", "dX", "poses_out", "patches_out"))
        # (the figure tests/test_gpu_solver_variants.py quotes for the fixtures: the construction has not made the system ill-conditioned)
        assert rel(r32["dX"], r64["dX"]) < 5e-3, (case, rel(r32["dX"], r64["dX"]))
        # the float32 storage of the new poses alone leaves room under the float64 routes' gate on the pose update (1e-5)
        free = np.arange(info["fixedp"], n_all)
        du = r64["poses_out"][free] - d["poses"][free]
        stored = r64["poses_out"][free].astype(np.float32).astype(np.float64) - d["poses"][free]
        assert np.linalg.norm(stored - du) / np.linalg.norm(du) < 0.7e-5, (case, np.linalg.norm(stored - du) / np.linalg.norm(du))


@pytest.mark.parametrize("case", list(mp.CASES))
def test_clamped_tracks_end_on_their_bound(case):
    """... exactly, in both precisions, and still with their start disparity moved 2 % towards the interior; an all-masked track
    has C = 0 and moves by the prior alone; a trackless patch is copied and clamped."""
    name, so, loss = mp.CASES[case]
    d, info = mp.problem(name)
    moved = dict(d, patches=d["patches"].copy())
    with_track = [p for p in info["clamp"] if p not in info["trackless"]]
    for p in with_track:
        x = moved["patches"][p, 2]
        if mp.LO <= x <= mp.HI:                                                 # (a start outside the clamp stays where it is)
            moved["patches"][p, 2] = np.float32(x * (0.98 if info["clamp"][p] == mp.HI else 1.02))
    for dtype in (np.float64, np.float32):
        for inp in (d, moved):
            out = mp.reference(case, dtype, inp)["patches_out"]
            for p, bound in info["clamp"].items():
                assert np.float32(out[p, 2]) == np.float32(bound), (case, dtype, p, out[p, 2])
            free = info["trackless"]
            assert np.array_equal(out[free, :2], inp["patches"][free, :2])
            assert np.array_equal(out[free, 2], np.clip(inp["patches"][free, 2], dtype(1e-3), dtype(10.0)))
    # C = 0: the prior alone, dZ = alpha (mono - d) / (alpha + lmbda)
    out = mp.reference(case)["patches_out"]
    for p in info["track_tags"].get("all_masked_track", []):
        want = d["patches"][p, 2] + 0.05 * (d["mono"][p] - d["patches"][p, 2]) / (0.05 + 1e-4)
        assert abs(out[p, 2] - min(want, 10.0)) < 1e-12 and out[p, 2] != d["patches"][p, 2]


def host_plan(d):
    return Plan(d["ii"], d["jj"], d["kk"], d["poses"].shape[0], d["patches"].shape[0], 1, upload=False)


def shares_tiles(plan, info):
    """every special track sits in a tile that also holds an ordinary track"""
    A = {k: plan.array(k) for k in ("trk_loc", "kx")}
    tile = A["trk_loc"] >> 6
    special = np.isin(A["kx"], info["special"])
    return all(t >= 0 and (~special[tile == t]).any() for t in tile[special]), tile[special]


def test_special_tracks_share_their_tiles_with_ordinary_ones():
    for name in ("base", "deep"):
        d, info = mp.problem(name)
        pl = host_plan(d)
        ok, tiles = shares_tiles(pl, info)
        assert ok, (name, tiles)
        pl.close()
    d, info = mp.problem("loose")
    pl = host_plan(d)
    loc, kx, lz = pl.array("trk_loc"), pl.array("kx"), pl.array("lz_trk")
    assert sorted(kx[loc < 0]) == sorted(kx[lz]) == sorted(info["hubs"])            # the hubs sit in no tile: ba_loose.hip steps them
    n_free = [len(set(d["jj"][d["kk"] == h]) | set(d["ii"][d["kk"] == h])) - 1 for h in info["hubs"]]
    assert min(n_free) > 64, n_free
    pl.close()


@pytest.mark.parametrize("case", [c for c, v in mp.CASES.items() if v[0] == "base"])
def test_plan_emulator_steps_the_base_problem_like_the_oracle(case):
    name, so, loss = mp.CASES[case]
    d, _ = mp.problem(name)
    pl = host_plan(d)
    em = emulate(pl, pl.arrays(), d, mp.wkey(so), structure_only=so, loss=loss)
    o = mp.reference(case)
    if not so:
        assert rel(np.tril(em["S_lower"]), np.tril(o["S"])) < 1e-10 and rel(em["y"], o["y"]) < 1e-10
        assert rel(em["dX"], o["dX"]) < 1e-7
    assert rel(em["patches_out"], o["patches_out"]) < 1e-10
    pl.close()
