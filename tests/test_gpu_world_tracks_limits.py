"""bt_world_tracks at its limits (include/batrack_projective.h, batrack_amd/csrc/world_tracks.hip): p x p patches whose
every pixel but the centre is a decoy, window lengths that leave parts of the four-way weight sum empty or shift `mid`,
one frame, one track, the tail block after a strided pass of the grid, both clamps of the window, NULL outputs, weights
that are NaN or sum to zero.

Reference and gates.  The reference is tests/world_util.np_world_tracks in float64 on the same float32-valued inputs.
The gates are measured per case from that restatement alone: e32 = rel_err(np_world_tracks(float32), float64) for points,
world and the disparity column; the kernel may be 2 x max(e32, 2^-23) away (the margin of test_gpu_world_tracks.py for a
fused kernel that composes the group actions in another order; the floor of one float32 unit because with one frame the
restatement's float32 disparity error is exactly 0).  (u, v): the project gate 2e-5 on |err| / (100 + |ref|) with more than
0.9 of the entries compared.  Finiteness agrees exactly, rows that are not live and rows past m are bit-equal to the input,
world rows past m keep a sentinel, two calls are bit-equal.  Every case prints its figures beside its gates."""
import ctypes

import numpy as np
import pytest
import torch

import world_util as wu
from batrack_amd.backend import projective_ops as pops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UV_GATE = 2e-5
FLOOR = 2.0 ** -23
SENTINEL = -12345.0
KEYS = ("poses", "intrinsics", "patches", "ix", "patches_local", "local_weights")
bits = lambda t: t.contiguous().view(torch.int32)
eq = lambda a, b: torch.equal(bits(a), bits(b))                  # bit for bit, NaN included


def restated(d, dt):
    return wu.np_world_tracks(*(d[k] if k == "ix" else d[k].astype(dt) for k in KEYS), int(d["m"]))[:3]


def run(d):
    """The kernel through pops.world_tracks on sentinel-filled outputs and a copy of the window buffer, twice (bit-equal);
    returns (points [m,3], world [NM,S,3], patches_local_out [NM,S,3]) as tensors."""
    g = wu.to_gpu(d, DEV)
    NM, S = d["patches_local"].shape[:2]
    outs = []
    for _ in range(2):
        pl = g["patches_local"].clone()
        points, world = torch.full((NM, 3), SENTINEL, device=DEV), torch.full((1, NM, S, 3), SENTINEL, device=DEV)
        p, w = pops.world_tracks(g["poses"], g["patches"], g["intrinsics"], g["ix"], pl, g["local_weights"], g["m"],
                                 points=points, world=world)
        assert p.data_ptr() == points.data_ptr() and w.data_ptr() == world.data_ptr()
        outs.append((points, world[0], pl[0]))
    assert all(eq(a, b) for a, b in zip(*outs)), "two calls differ"
    return outs[0]


def check(d, desc):
    """Run the kernel on `d` and hold it to the float64 restatement under the gates of the float32 restatement."""
    m = int(d["m"])
    NM = d["patches_local"].shape[0]
    ref, r32 = restated(d, np.float64), restated(d, np.float32)
    live = np.nan_to_num(d["local_weights"][:m].astype(np.float64).sum(1), nan=-1.0) > 0
    e = wu.parity_figures(tuple(a.astype(np.float64) for a in r32), ref, m, live)
    points, world, pl = run(d)
    np64 = lambda t: t.cpu().numpy().astype(np.float64)
    got = (np64(points[:m]), np64(world), np64(pl))
    got[1][m:] = 0.0                                             # the restatement has zeros past m; the sentinel is asserted below
    f = wu.parity_figures(got, ref, m, live)
    gates = {k: 2.0 * max(e[k], FLOOR) for k in ("points", "world", "disp")}
    msg = (f"{desc}: m {m} live {int(live.sum())} | " + " | ".join(f"{k} err {f[k]:.3e} gate {gates[k]:.3e} (e32 {e[k]:.3e})" for k in gates)
           + f" | uv err {f['uv']:.3e} gate {UV_GATE:.0e} share {f['uv_share']:.2f} (restatement's float32: {e['uv']:.3e}, share {e['uv_share']:.2f})")
    print(msg)
    assert e["finite"] and e["rest"], msg                        # the restatement with itself
    assert f["finite"], msg
    assert f["rest"], msg
    inp = torch.as_tensor(d["patches_local"], device=DEV)
    dead = torch.as_tensor(np.pad(~live, (0, NM - m), constant_values=True), device=DEV)
    assert eq(pl[dead], inp[dead]), msg                          # not live or past m: bit-equal to the input
    assert bool((world[m:] == SENTINEL).all()) and bool((points[m:] == SENTINEL).all()), msg
    if m < NM:
        assert not bool((world[:m] == SENTINEL).any()), msg
    if live.any():
        assert e["uv"] < UV_GATE and e["uv_share"] > 0.9, msg
        assert f["uv"] < UV_GATE and f["uv_share"] > 0.9, msg
    for k in gates:
        assert f[k] <= gates[k], msg
    return points, world, pl, live


@pytest.mark.parametrize("S_local", [1, 2, 3, 4, 8, 129])
def test_window_lengths(S_local):
    """S_local < 4 leaves parts of the four-way weight sum empty, an even S_local shifts mid, 129 > 2 N clamps most slots."""
    d = wu.random_inputs(12, 16, 4, 11, seed=100 + S_local, S_local=S_local)
    assert d["patches_local"].shape == (192, S_local, 3)
    live = check(d, f"S_local {S_local}")[3]
    assert live.any() and not live.all()


@pytest.mark.parametrize("p", [2, 3, 64])
def test_patch_sizes_with_decoys(p):
    """Every pixel but the centre (p/2, p/2) is a decoy in +-1000: a wrong centre index (p/2)(p+1) or plane stride p*p moves
    x, y or d by hundreds."""
    d = wu.random_inputs(12, 16, 4, 11, seed=200 + p, S_local=7, p=p)
    assert d["patches"].shape == (192, 3, p, p)
    check(d, f"p {p}")


def test_one_frame():
    """N = 1: every window frame clamps to frame 0."""
    d = wu.random_inputs(1, 70, 4, 1, seed=301, p=3)
    assert d["m"] == 70 and d["poses"].shape == (1, 7)
    check(d, "N 1, M 70, p 3")


@pytest.mark.parametrize("m,first_live", [(1, True), (1, False), (63, True), (64, True), (65, True)])
def test_track_counts_around_one_block(m, first_live):
    d = wu.random_inputs(12, 16, 4, 11, seed=400 + m)
    d["m"] = m
    S = d["local_weights"].shape[1]
    d["local_weights"][0] = 0.0
    if first_live:
        d["local_weights"][0, (S + 1) // 2 - 1] = 0.5
    live = check(d, f"m {m}, track 0 {'live' if first_live else 'not live'}")[3]
    assert bool(live[0]) == first_live


def test_tail_block_after_a_strided_pass():
    """m = 2048 * 64 + 1: the grid of 2048 workgroups takes 64 tracks each, then block 2048 — one track — falls to
    workgroup 0 in its second trip."""
    N, M, m = 513, 256, 2048 * 64 + 1
    d = wu.random_inputs(N, M, 4, N, seed=500, S_local=3)
    assert N * M > m
    d["m"] = m
    d["local_weights"][m - 1] = (0.0, 0.5, 0.0)                  # the tail track is live: it writes its patches_local row
    d["local_weights"][m] = (0.0, 0.5, 0.0)                      # and the first track past m would, if it were taken
    live = check(d, f"m {m}")[3]
    assert live[-1]


@pytest.mark.parametrize("end", ["first", "last"])
def test_source_frames_at_the_ends_of_the_buffer(end):
    """S_local = 23 (mid 11) in a buffer of 6 frames, every track's own frame the first / the last: the lower clamp acts
    on 11 / 6 slots of every track and the upper one on 6 / 11, 17 of 23 together."""
    d = wu.random_inputs(6, 32, 12, 6, seed=600)
    N = d["poses"].shape[0]
    d["ix"][:] = 0 if end == "first" else N - 1
    j = d["ix"][:, None] + np.arange(23)[None] - 11
    assert ((j < 0) | (j > N - 1)).mean() == 17 / 23 and (j < 0).any() and (j > N - 1).any()
    check(d, f"every source frame {d['ix'][0]} of {N}, S_local 23")


def _raw(d, g, points, world):
    """bt_world_tracks through the C ABI; `points` / `world`: a tensor or None (NULL).  Returns the window buffer."""
    from batrack_amd import _lib
    pl = g["patches_local"].clone()
    NM, S = d["patches_local"].shape[:2]
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    P, K, pat, lw = (g[k].reshape(s).contiguous() for k, s in (("poses", (-1, 7)), ("intrinsics", (-1, 4)),
                                                                ("patches", (NM, 3, -1)), ("local_weights", (NM, S))))
    rc = _lib.lib().bt_world_tracks(ptr(P), P.shape[0], ptr(K), ptr(pat), NM, pat.shape[-1], ptr(g["ix"]), ptr(pl), ptr(lw), S,
                                    int(d["m"]), ptr(points), ptr(world), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.BT_OK, rc
    return pl[0]


def test_null_outputs():
    """points == NULL and world == NULL, which the header allows: what is still written is bit-equal to the full call."""
    d = wu.random_inputs(12, 16, 4, 11, seed=700, p=3)
    points, world, pl, live = check(d, "NULL outputs: the full call")
    g = wu.to_gpu(d, DEV)
    NM, S = d["patches_local"].shape[:2]
    new = lambda *s: torch.full(s, SENTINEL, device=DEV)
    w1 = new(NM, S, 3)
    pl1 = _raw(d, g, None, w1)
    assert eq(w1, world) and eq(pl1, pl)
    p2 = new(NM, 3)
    pl2 = _raw(d, g, p2, None)
    assert eq(p2, points) and eq(pl2, pl)
    pl3 = _raw(d, g, None, None)
    assert eq(pl3, pl)
    rows = torch.as_tensor(np.flatnonzero(live), device=DEV)
    assert live.any() and not eq(pl3[rows], g["patches_local"][0][rows])      # the live rows were overwritten


def test_nan_and_cancelling_weights_are_not_live():
    d = wu.random_inputs(12, 16, 4, 11, seed=800)
    m, S = d["m"], d["local_weights"].shape[1]
    was = np.flatnonzero(d["local_weights"][:m].sum(1) > 0)
    nan_k, zero_k = was[:6], was[6:12]
    for n, k in enumerate(nan_k):
        d["local_weights"][k, n % S] = np.nan                    # in each of the four partial sums in turn
    d["local_weights"][zero_k] = 0.0
    for n, k in enumerate(zero_k):
        d["local_weights"][k, n % S], d["local_weights"][k, (n + 1 + n % 3) % S] = 0.5, -0.5      # exact in any order
    points, world, pl, live = check(d, "NaN weights and weights that cancel")
    changed = np.concatenate([nan_k, zero_k])
    assert not live[changed].any() and live.any()
    rows = torch.as_tensor(changed, device=DEV)
    assert eq(pl[rows], torch.as_tensor(d["patches_local"], device=DEV)[rows])
