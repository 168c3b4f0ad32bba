"""BA problems whose edges and tracks sit on purpose on either side of every per-edge and per-track decision of the step
(batrack_amd/csrc/ba_edge.hpp: edge_eval<float>, edge_eval<double>, edge_eval_mixed; ba_update.hpp: clamp_disp, new_disp,
update_rest), shared by tests/test_edge_masks_cpu.py (which checks the construction against the oracle) and
tests/test_gpu_edge_masks.py (which steps them through every Jacobian kernel):

    iz  = 1 / max(Z, 1e-2)          dj = |Z| > 0.2 ? 1/Z : 0
    vld = (Z > 0.2) * (|r| < 250) * (b0 < u < b2 and b1 < v < b3)
    W   = vld * w * robust(r)       d' = clamp(d + Q (w' - tot), 1e-3, 10)

Pure numpy + oracle.  Inputs are built in float64, rounded to float32 and stated as float64, as edge_problems.problem does.

The poses are world-to-camera: seen from source frame 0 (identity), a point of disparity d has Z = 1 + t_z d in camera k, with
t_z = -0.1 k (frame 1: -0.125, and the identity quaternion, so that d = 8 gives Z = 0 exactly in every precision).  That is
also why the `clamp_hi` track is the one special track whose source is not frame 0: from frame 0 a point of disparity 9.9 lies
behind every other camera (Z = 1 - 0.1 k 9.9 < 0), so a track with VALID edges near the upper bound has to look back from the
last frame (t_z > 0); it shares that frame's tile with ordinary tracks just the same.  And the prior alone cannot push a track
that has well-weighted edges (C = sum W Jz^2 ~ 1e3 against alpha = 0.05): the clamp tracks' targets are the reprojection of a
disparity past the bound, and the prior pulls the same way.

The seeds.  The targets are the state's own reprojection plus noise, so the pose update of the base graph is small (|update|
1e-3 .. 5e-3 over its four free poses) and the float32 storage of poses_out alone — the oracle's float64 poses_out rounded to
float32 — costs gpu_util.update_err 1e-5 .. 3e-5 at most seeds: the project's gate on the pose update (1e-5) cannot be met
there by any kernel.  The seeds are ones at which that rounding leaves room under the gate (6e-6 and less) and at which the
oracle's float32 run stays within 5e-3 of its float64 run on dX for every case, `deep` (nine times the float32 additions)
included; tests/test_edge_masks_cpu.py asserts both, so that a change to the builder cannot silently lose either.
"""
import numpy as np

import oracle

K4 = np.array([500.0, 500.0, 320.0, 240.0])
BOUNDS = np.array([0.0, 0.0, 640.0, 480.0])
F32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
LO, HI = float(np.float32(1e-3)), 10.0

# margins of the construction (tests/test_edge_masks_cpu.py asserts them on every edge, tagged or not)
M_Z02, M_UV, M_R, M_KNEE = 0.05, 0.5, 0.5, 0.05


# ------------------------------------------------------------------ geometry in numpy
def rot(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2*(y*y + z*z), 2*(x*y - z*w), 2*(x*z + y*w)],
                     [2*(x*y + z*w), 1 - 2*(x*x + z*z), 2*(y*z - x*w)],
                     [2*(x*z - y*w), 2*(y*z + x*w), 1 - 2*(x*x + y*y)]])


def point_in_target(poses, patch, i, j):
    """(X, Y, Z) of patch (x, y, d) of frame i in camera j (projective_ops.py:61-66), float64 numpy"""
    Ri, Rj = rot(poses[i, 3:]), rot(poses[j, 3:])
    R = Rj @ Ri.T
    t = poses[j, :3] - R @ poses[i, :3]
    X0 = np.array([(patch[0] - K4[2]) / K4[0], (patch[1] - K4[3]) / K4[1], 1.0])
    return R @ X0 + t * patch[2]


def project(poses, patch, i, j):
    """u, v, Z, with the reprojection's own clamp of Z (projective_ops.py:43-45)"""
    X, Y, Z = point_in_target(poses, patch, i, j)
    iz = 1.0 / max(Z, 1e-2)
    return K4[0] * iz * X + K4[2], K4[1] * iz * Y + K4[3], Z


def edge_z(d):
    """Z of every edge's point in its target camera (float64 numpy on the problem's float32-rounded inputs)"""
    return np.array([point_in_target(d["poses"], d["patches"][k], i, j)[2] for i, j, k in zip(d["ii"], d["jj"], d["kk"])])


def z_clear(Z):
    """Z is 0.05 or more from +-0.2 (vld's and dj's threshold) and a factor of 2 from 1e-2 (iz's clamp), or it is the exact zero"""
    return (abs(abs(Z) - 0.2) >= M_Z02) and (Z >= 2e-2 or Z <= 5e-3)


def uv_clear(u, v, m=M_UV):
    return min(abs(u - BOUNDS[0]), abs(u - BOUNDS[2]), abs(v - BOUNDS[1]), abs(v - BOUNDS[3])) >= m


def inside(u, v):
    return BOUNDS[0] < u < BOUNDS[2] and BOUNDS[1] < v < BOUNDS[3]


# ------------------------------------------------------------------ the frames
def make_poses(N, step_x, step_z, rng):
    poses = np.zeros((N, 7)); poses[:, 6] = 1.0
    poses[:, 0] = step_x * np.arange(N)
    poses[:, 2] = -step_z * np.arange(N)
    q = 0.01 * rng.standard_normal((N, 4)) + np.array([0, 0, 0, 1.0])
    poses[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    poses[0, 3:] = poses[1, 3:] = (0, 0, 0, 1.0)          # frames 0 and 1: the identity, exactly
    poses[1, 2] = -1.25 * step_z                          # base graph: -0.125, so that 1 + t_z 8 = 0 exactly
    return F32(poses)


def search(poses, i, js, cands, pred):
    """The first candidate patch (x, y, d), float32-rounded, whose projections [(u, v, Z) per frame of js] satisfy pred"""
    for c in cands:
        c = F32(c)
        pr = [project(poses, c, i, j) for j in js]
        if all(z_clear(Z) for _, _, Z in pr) and all(uv_clear(u, v, 2 * M_UV) for u, v, _ in pr) and pred(pr):
            return c
    raise AssertionError("no candidate patch satisfies the construction")


def side_pred(side, out):
    """out=True: every frame sees the point well in front (Z > 0.25); it leaves through `side` alone in at least one frame and stays
    inside in at least one other.  out=False: inside and within 8 px of `side` in at least one frame."""
    def gone(u, v):
        return {"l": u < BOUNDS[0], "r": u > BOUNDS[2], "t": v < BOUNDS[1], "b": v > BOUNDS[3]}[side]

    def only(u, v):     # leaves through that side and no other
        fails = [u <= BOUNDS[0], u >= BOUNDS[2], v <= BOUNDS[1], v >= BOUNDS[3]]
        return gone(u, v) and sum(fails) == 1

    def near(u, v):
        return inside(u, v) and {"l": u - BOUNDS[0], "r": BOUNDS[2] - u, "t": v - BOUNDS[1], "b": BOUNDS[3] - v}[side] <= 8.0

    def pred(pr):
        if not all(Z > 0.25 for _, _, Z in pr):
            return False
        if out:
            return all(inside(u, v) or only(u, v) for u, v, _ in pr) and any(only(u, v) for u, v, _ in pr) and any(inside(u, v) for u, v, _ in pr)
        return any(near(u, v) for u, v, _ in pr)
    return pred, near


def border_patch(side, inset):
    """candidates (x, y, d): `inset` px inside `side`, the other coordinate a little around the centre, disparities from far to near"""
    for off in (0.0, -60.0, 60.0, -120.0, 120.0):
        for dd in np.geomspace(0.01, 2.5, 300):
            yield {"l": (inset, 240.0 + off, dd), "r": (640.0 - inset, 240.0 + off, dd),
                   "t": (320.0 + off, inset, dd), "b": (320.0 + off, 480.0 - inset, dd)}[side]


# ------------------------------------------------------------------ assembling a problem
class Builder:
    def __init__(self, N, step_x, step_z, p_tot, seed):
        self.rng = np.random.default_rng(seed)
        self.N, self.p_tot = N, p_tot
        self.poses = make_poses(N, step_x, step_z, self.rng)
        self.patches = np.zeros((p_tot, 3))
        self.d_true = {}                 # patch -> the disparity its targets are the reprojection of (default: its own)
        self.mono = {}                   # patch -> its prior (default: 1.05 d)
        self.ii, self.jj, self.kk = [], [], []
        self.ordinary = []               # (patch, source frame, target frames): redrawn until every edge is clear of the thresholds
        self.track_tags = {}             # tag -> [patch]
        self.edge_tags = {}              # tag -> [(patch, target frame, expected valid)]
        self.shift = {}                  # (patch, target frame) -> (du, dv): target = reprojection + this, no noise

    def track(self, patch, i, js, xyd=None, tag=None):
        if xyd is not None:
            self.patches[patch] = F32(xyd)
            assert all(z_clear(point_in_target(self.poses, self.patches[patch], i, j)[2]) for j in js), "a special track is near a threshold on Z"
        else:
            self.ordinary.append((patch, i, list(js)))
        for j in js:
            self.ii.append(i); self.jj.append(j); self.kk.append(patch)
        if tag:
            self.track_tags.setdefault(tag, []).append(patch)

    def tag_edges(self, tag, patch, js, valid):
        self.edge_tags.setdefault(tag, []).extend((patch, j, valid) for j in js)

    def draw_ordinary(self, todo):
        """x, y, d of the ordinary patches `todo`, redrawn until every edge of each is clear of every threshold by the margins"""
        for patch, i, js in todo:
            for _ in range(1000):
                c = F32((self.rng.uniform(120, 520), self.rng.uniform(90, 390), self.rng.uniform(0.2, 0.8)))
                pr = [project(self.poses, c, i, j) for j in js]
                if all(z_clear(Z) and Z > 0.25 for _, _, Z in pr) and all(uv_clear(u, v, 2 * M_UV) for u, v, _ in pr):
                    self.patches[patch] = c
                    break
            else:
                raise AssertionError("no ordinary patch clear of the thresholds")

    def finish(self, repeat=1):
        rng = self.rng
        self.draw_ordinary(self.ordinary)
        # patches that carry no track and were given no value: ordinary numbers
        free = sorted(set(range(self.p_tot)) - set(self.kk))
        for p in free:
            if not self.patches[p].any():
                self.patches[p] = F32((rng.uniform(100, 540), rng.uniform(80, 400), rng.uniform(0.2, 1.0)))
        ii, jj, kk = (np.asarray(a, np.int64) for a in (self.ii, self.jj, self.kk))
        perm = rng.permutation(ii.size)                    # (the caller's order is not the planner's)
        ii, jj, kk = ii[perm], jj[perm], kk[perm]
        E = ii.size
        mono = self.patches[:, 2] * 1.05
        for p, m in self.mono.items():
            mono[p] = m
        d = dict(poses=self.poses, patches=F32(self.patches), mono=F32(mono), intrinsics=F32(np.tile(K4, (self.N, 1))),
                 ii=ii, jj=jj, kk=kk, bounds=BOUNDS.copy())
        # targets: the float64 reprojection of the state (of d_true where a track is to be pushed) plus 0.5 px of noise, no component
        # of which lies within 0.1 of the huber knee; the tagged residuals are exact shifts without noise
        aim = d["patches"].copy()
        for p, dt in self.d_true.items():
            aim[p, 2] = dt
        e = oracle.edges(d["poses"], aim, d["intrinsics"], np.zeros((E, 3)), np.ones((E, 2)), ii, jj, kk, d["bounds"])
        push = e["coords"] - oracle.edges(d["poses"], d["patches"], d["intrinsics"], np.zeros((E, 3)), np.ones((E, 2)), ii, jj, kk, d["bounds"])["coords"]
        noise = rng.normal(0, 0.5, (E, 2))
        for _ in range(100):
            bad = np.abs(np.abs(push + noise) - 1.0) < 0.1
            if not bad.any():
                break
            noise[bad] = rng.normal(0, 0.5, int(bad.sum()))
        key = {(int(k), int(j)): n for n, (k, j) in enumerate(zip(kk, jj))}
        for (p, j), s in self.shift.items():
            noise[key[(p, j)]] = s
        t3 = np.zeros((E, 3)); t3[:, :2] = e["coords"] + noise
        d["targets3"] = F32(t3)
        d["weights_pose"] = F32(rng.uniform(0.5, 1.0, (E, 2)))
        d["weights"] = F32(rng.uniform(0.5, 1.0, (E, 2)))
        edge_tags = {t: (np.array([key[(p, j)] for p, j, _ in v], np.int64), np.array([x for _, _, x in v], np.float64))
                     for t, v in self.edge_tags.items()}
        if repeat > 1:        # every observation `repeat` times (deep() of tests/test_gpu_jacobian_kernels.py) at 1 / repeat of its
            # weight: the same normal equations as the graph it repeats, so as well conditioned against the damping ep
            for name in ("ii", "jj", "kk", "targets3", "weights", "weights_pose"):
                d[name] = np.ascontiguousarray(np.repeat(d[name], repeat, axis=0))
            d["weights"], d["weights_pose"] = F32(d["weights"] / repeat), F32(d["weights_pose"] / repeat)
            edge_tags = {t: ((repeat * ed[:, None] + np.arange(repeat)).reshape(-1), np.repeat(v, repeat)) for t, (ed, v) in edge_tags.items()}
        tagged = np.zeros(len(d["ii"]), bool)
        for ed, _ in edge_tags.values():
            tagged[ed] = True
        special = sorted({p for v in self.track_tags.values() for p in v})
        info = dict(edge_tags=edge_tags, track_tags={t: list(v) for t, v in self.track_tags.items()}, tagged=tagged,
                    special=special, trackless=free, fixedp=1)
        return d, info


def out_track(b, patch, i, js, side):
    pred, _ = side_pred(side, True)
    c = search(b.poses, i, js, border_patch(side, 3.0), pred)
    b.track(patch, i, js, c, tag="out_" + side)
    pr = [project(b.poses, c, i, j) for j in js]
    b.tag_edges("out_" + side, patch, [j for j, (u, v, _) in zip(js, pr) if not inside(u, v)], 0.0)


def in_track(b, patch, i, js, side):
    pred, near = side_pred(side, False)
    c = search(b.poses, i, js, border_patch(side, 6.0), pred)
    b.track(patch, i, js, c, tag="in_" + side)
    pr = [project(b.poses, c, i, j) for j in js]
    b.tag_edges("in_" + side, patch, [j for j, (u, v, _) in zip(js, pr) if near(u, v)], 1.0)


# positions of the ordinary tracks among frame 0's 24 (spread, so that a tile of 16 tracks holds some as well)
BASE_ORDINARY0 = (2, 8, 14, 20)
BASE_M = 24


def base(seed=963, repeat=1):
    """5 frames x 24 tracks, every track seen from the four other frames (480 edges), fixedp = 1, 8 patches without a track"""
    N, M = 5, BASE_M
    b = Builder(N, 0.05, 0.1, N * M + 8, seed)
    others = lambda i: [j for j in range(N) if j != i]
    js = others(0)
    slots = iter(p for p in range(M) if p not in BASE_ORDINARY0)
    Zs = lambda p: [point_in_target(b.poses, b.patches[p], 0, j)[2] for j in js]
    # --- Z: on a camera's plane, thin, behind, mixed
    p = next(slots); b.track(p, 0, js, (300.0, 200.0, 8.0), "z_zero"); b.tag_edges("z_zero", p, [1], 0.0)
    b.track_tags.setdefault("all_masked_track", []).append(p)                       # (frames 2..4: behind)
    p = next(slots); b.track(p, 0, js, (350.0, 260.0, 7.2), "z_thin"); b.tag_edges("z_thin", p, [1], 0.0)       # Z_1 = 0.1: dj = 0
    b.track_tags["z_thin_dj"] = [p]
    p = next(slots); b.track(p, 0, js, (280.0, 220.0, 7.968), "z_thin"); b.tag_edges("z_thin", p, [1], 0.0)     # Z_1 = 0.004: iz clamped
    b.track_tags["z_thin_iz"] = [p]
    p = next(slots); b.track(p, 0, js, (330.0, 230.0, 9.0), "z_behind"); b.tag_edges("z_behind", p, [2, 3, 4], 0.0)   # Z = -0.8, -1.7, -2.6
    b.track_tags.setdefault("all_masked_track", []).append(p)                       # (frame 1: Z = -0.125)
    # ... and behind camera 3 ON its axis (Z = -0.29, d = 4.3): the clamped reprojection lands mid-image next to its target, so that Z > 0.2
    # is the one comparison that fails there (a mask on |Z| would let the edge in with full weight)
    R3, t3 = rot(b.poses[3, 3:]), b.poses[3, :3]
    a3, b3, dd = np.linalg.solve(np.column_stack([R3[:, :2], t3]), np.array([0.0, 0.0, -0.29]) - R3[:, 2])
    p = next(slots); b.track(p, 0, js, (K4[2] + K4[0] * a3, K4[3] + K4[1] * b3, dd), "z_behind_axis")
    b.tag_edges("z_behind_axis", p, [3], 0.0)
    p = next(slots); b.track(p, 0, js, (170.0, 260.0, 3.2), "z_mixed")             # Z = 0.6, 0.36 | 0.04, -0.28
    b.tag_edges("z_mixed", p, [1, 2], 1.0); b.tag_edges("z_mixed", p, [3, 4], 0.0)
    # --- the bounds, one side at a time
    for side in "lrtb":
        out_track(b, next(slots), 0, js, side)
    for side in "lrtb":
        in_track(b, next(slots), 0, js, side)
    # --- |r| on either side of 250 px, along an axis and along the diagonal
    for tag, s_axis, s_diag, valid in (("r_249", 249.0, 176.0, 1.0), ("r_251", 251.0, 178.0, 0.0)):
        p = next(slots); b.track(p, 0, js, (300.0 + 40 * valid, 250.0, 0.4), tag)
        b.shift[(p, 1)] = (s_axis, 0.0); b.shift[(p, 2)] = (s_diag, s_diag)
        b.tag_edges(tag, p, [1, 2], valid)
    # --- the huber knee: both signs of 0.9 and 1.1 on both components
    p = next(slots); b.track(p, 0, js, (360.0, 200.0, 0.5), "knee")
    for j, s in zip(js, ((0.9, -1.1), (-0.9, 1.1), (1.1, 0.9), (-1.1, -0.9))):
        b.shift[(p, j)] = s
    b.tag_edges("knee", p, js, 1.0)
    # --- the clamp: tracks with valid edges pushed through either end (their targets are the reprojection of a disparity past it)
    p = next(slots); b.track(p, 0, js, (300.0, 300.0, 1.2e-3), "clamp_lo"); b.d_true[p] = -0.1
    b.tag_edges("clamp_lo", p, js, 1.0)
    p = (N - 1) * M + 5; hi_js = others(N - 1)
    # --- start disparities outside the clamp, on tracks with edges (12: behind every camera, the prior alone moves it) ...
    q = next(slots); b.track(q, 0, js, (310.0, 180.0, 12.0), "start_out_hi")
    b.track_tags.setdefault("all_masked_track", []).append(q)
    q = next(slots); b.track(q, 0, js, (340.0, 280.0, 1e-4), "start_out_lo"); b.d_true[q] = -0.1
    assert next(slots, None) is None
    for k in BASE_ORDINARY0:
        b.track(k, 0, js)
    for i in range(1, N):
        for k in range(i * M, (i + 1) * M):
            if k == p:
                b.track(p, N - 1, hi_js, (470.0, 250.0, 9.9), "clamp_hi"); b.d_true[p] = 11.0; b.mono[p] = 11.0
                b.tag_edges("clamp_hi", p, hi_js, 1.0)
            else:
                b.track(k, i, others(i))
    # ... and on patches without a track
    b.patches[N * M] = (123.0, 45.0, 12.0); b.patches[N * M + 1] = (67.5, 89.25, 1e-4)
    d, info = b.finish(repeat)
    info["clamp"] = {p: HI, info["track_tags"]["clamp_lo"][0]: LO, info["track_tags"]["start_out_hi"][0]: HI,
                     info["track_tags"]["start_out_lo"][0]: LO, N * M: HI, N * M + 1: LO}
    info["start_out_trackless"] = [N * M, N * M + 1]
    return d, info


def deep(seed=963):
    """The base graph with every observation 9 times: a forced k_stream takes it, the special edges on several slots of a lane"""
    return base(seed, repeat=9)


def loose(seed=4):
    """70 frames (a fifth of the base graph's spacing), 4 ordinary tracks per frame seen from the 4 nearest frames, and three hub
    tracks seen from all 69 other frames (more than 64 free cameras: they fit no tile): one behind most of its cameras, one whose
    edges leave through the right and the top border, one pushed through the upper clamp."""
    N, M = 70, 4
    b = Builder(N, 0.01, 0.02, N * M + 3 + 2, seed)
    for i in range(N):
        js = sorted(sorted((j for j in range(N) if j != i), key=lambda j: (abs(j - i), j))[:4])
        for k in range(i * M, (i + 1) * M):
            b.track(k, i, js)
    h0, h1, h2 = N * M, N * M + 1, N * M + 2
    # hub behind most cameras: from frame 0, Z = 1 - 0.02 k d falls through 0.2, 1e-2, 0 and -0.2 in steps wider than the margins
    js = list(range(1, N))
    c = search(b.poses, 0, js, ((250.0, 215.0, dd) for dd in np.arange(5.0, 9.5, 0.01)),
               lambda pr: sum(Z > 0.25 and inside(u, v) for u, v, Z in pr) >= 4 and sum(Z < -0.5 for _, _, Z in pr) >= 20)
    b.track(h0, 0, js, c, "hub_z_mixed")
    pr = [project(b.poses, c, 0, j) for j in js]
    b.tag_edges("hub_z_mixed", h0, [j for j, (u, v, Z) in zip(js, pr) if Z > 0.2 and inside(u, v)], 1.0)
    b.tag_edges("hub_z_mixed", h0, [j for j, (u, v, Z) in zip(js, pr) if Z < 0.2], 0.0)
    # hub leaving through two borders: from the middle frame, near the top right corner
    mid = N // 2
    js = [j for j in range(N) if j != mid]

    def two_sides(pr):
        r = sum(u > BOUNDS[2] and inside(u - 640.0 + 1.0, v) for u, v, _ in pr)      # through the right border alone
        t = sum(v < BOUNDS[1] for u, v, _ in pr)
        return all(Z > 0.25 for _, _, Z in pr) and r >= 2 and t >= 2 and sum(inside(u, v) for u, v, _ in pr) >= 20
    c = search(b.poses, mid, js, ((x, y, dd) for dd in np.arange(0.2, 0.6, 0.01) for x in (600.0, 590.0, 610.0) for y in (25.0, 35.0, 45.0)), two_sides)
    b.track(h1, mid, js, c, "hub_out")
    pr = [project(b.poses, c, mid, j) for j in js]
    b.tag_edges("hub_out", h1, [j for j, (u, v, _) in zip(js, pr) if not inside(u, v)], 0.0)
    b.tag_edges("hub_in", h1, [j for j, (u, v, _) in zip(js, pr) if inside(u, v)], 1.0)
    # hub pushed through the upper clamp: looks back from the last frame, valid in all 69
    js = list(range(N - 1))
    c = search(b.poses, N - 1, js, ((x, y, 9.9) for x in (470.0, 400.0, 330.0, 260.0, 190.0) for y in (250.0, 190.0, 310.0, 130.0, 370.0)),
               lambda pr: all(Z > 0.25 and inside(u, v) for u, v, Z in pr))
    b.track(h2, N - 1, js, c, "clamp_hi"); b.d_true[h2] = 11.0; b.mono[h2] = 11.0
    b.tag_edges("clamp_hi", h2, js, 1.0)
    b.patches[N * M + 3] = (123.0, 45.0, 12.0); b.patches[N * M + 4] = (67.5, 89.25, 1e-4)
    d, info = b.finish()
    info["hubs"] = [h0, h1, h2]
    info["clamp"] = {h2: HI, N * M + 3: HI, N * M + 4: LO}
    info["start_out_trackless"] = [N * M + 3, N * M + 4]
    return d, info


BUILDERS = {"base": base, "deep": deep, "loose": loose}
# (problem, structure-only, loss): each problem as a pose+structure step (weights_pose) and as a structure-only step (weights);
# the base graph also under the two other losses
CASES = {"base": ("base", False, "huber"), "base_so": ("base", True, "huber"), "base_cauchy": ("base", False, "cauchy"),
         "base_trivial": ("base", False, "trivial"), "deep": ("deep", False, "huber"), "deep_so": ("deep", True, "huber"),
         "loose": ("loose", False, "huber"), "loose_so": ("loose", True, "huber")}

_BUILT = {}


def problem(name):
    """(inputs, info) of BUILDERS[name], built once per process; treat as read-only"""
    if name not in _BUILT:
        _BUILT[name] = BUILDERS[name]()
    return _BUILT[name]


def wkey(so):
    return "weights" if so else "weights_pose"


def reference(case, dtype=np.float64, d=None):
    """oracle.ba_step of a case (of the inputs d instead of the problem's own, if given), with the reduced system"""
    name, so, loss = CASES[case]
    if d is None:
        d = problem(name)[0]
    return oracle.ba_step(d["poses"], d["patches"], d["mono"], d["intrinsics"], d["targets3"], d[wkey(so)], d["ii"], d["jj"], d["kk"],
                          d["bounds"], fixedp=1, structure_only=so, loss=loss, dtype=dtype, want_system=not so)


def oracle_edges(case, dtype=np.float64):
    name, so, loss = CASES[case]
    d = problem(name)[0]
    return oracle.edges(d["poses"], d["patches"], d["intrinsics"], d["targets3"], d[wkey(so)], d["ii"], d["jj"], d["kk"], d["bounds"],
                        loss=loss, dtype=dtype)
