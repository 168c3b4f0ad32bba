"""The three stages of include/batrack_keyframe.h through the raw C ABI (ctypes), at the sizes where their code changes path:
the compaction against numpy's boolean masks from no edge to more tiles than one pass of the scan takes, the decision with
its selected edges in none, one, several workgroups and in the last partial wave, the row shift over every unit width.
Nothing here provokes a fault: out-of-range indices are answered with NaN by design, as in bt_reproject."""
import ctypes

import numpy as np
import pytest
import torch

import keyframe_util as ku
from batrack_amd import _lib, graphgen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# A mean flow magnitude against its float64 evaluation, in pixels.  A flow is the norm of a difference of two pixel
# coordinates, each the end of a chain of about 30 float32 operations (normalisation, two rotations, projection) whose result
# is below 320 px here; allowing every operation of the longer chain half an ulp of that result and the two coordinates'
# errors to add gives 2 * 30 * 2^-25 * 320 px = 5.7e-4 px.  A mean of one edge has nothing to average it down, so the bound
# is the same for every count.  (The decisions are tested 0.5 px from the threshold: a thousand times that.)
MAG_TOL_PX = 2 * 30 * 2.0 ** -25 * 320
CANARY = -7777


def lib():
    return _lib.lib()


def workspace(E, removed=0):
    """A workspace whose status the test writes: removed as given, the other fields a pattern no stage writes by accident."""
    ws = torch.full((lib().bt_keyframe_workspace_bytes(E) // 8 + 4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    ws[0] = removed
    return ws


def status(ws):
    torch.cuda.synchronize()
    return _lib.KeyframeStatus.from_buffer_copy(ws[:4].cpu().numpy().tobytes())


def stream():
    return torch.cuda.current_stream().cuda_stream


def prune_sizes():
    tile, span = lib().bt_edges_prune_tile(), lib().bt_edges_prune_scan_span()
    return [0, 1, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 3 * tile + 17, tile * (span + 1) + 3]


K, N_FR, M, WINDOW = 35, 40, 4, 10
PATTERNS = ("all", "none", "first", "last", "alternating", "half")


def prune_edges(E, pattern, removed, rng):
    """Edges whose fate under (k, n, M, window) above follows `pattern`; dropped edges cycle through every reason to drop."""
    want = dict(all=np.ones(E, bool), none=np.zeros(E, bool), first=np.arange(E) == 0, last=np.arange(E) == E - 1,
                alternating=np.arange(E) % 2 == 0, half=rng.random(E) < 0.5)[pattern]
    lim = N_FR - WINDOW - (1 if removed else 0)                     # the oldest source that stays, in the numbers after the removal
    young = np.array([f for f in range(N_FR) if (f - (f > K) if removed else f) >= lim and not (removed and f == K)])
    ii = young[rng.integers(0, young.size, E)]
    jj = np.array([f for f in range(N_FR) if f != K])[rng.integers(0, N_FR - 1, E)]
    drop = np.flatnonzero(~want)
    reason = np.arange(drop.size) % (3 if removed else 1)
    old = rng.integers(0, lim, drop.size)
    ii[drop] = np.where(reason == 0, old, np.where(reason == 1, K, ii[drop]))
    jj[drop] = np.where(reason == 2, K, jj[drop])
    if not removed:                                                  # with the frame kept, edges at k stay: put some among the kept
        kept = np.flatnonzero(want)
        jj[kept[::5]] = K
    kk = ii * M + rng.integers(0, M, E)
    return ii.astype(np.int64), jj.astype(np.int64), kk.astype(np.int64), want


@pytest.mark.parametrize("E", prune_sizes())
def test_prune_against_numpy_masks(E):
    L = lib()
    rng = np.random.default_rng(E)
    pad = 5
    e = np.arange(E, dtype=np.float32)                               # payload rows encode their edge index (exact below 2^24)
    pay = [np.stack([e, e + 0.25, e + 0.5], 1), np.stack([e, -e], 1), np.stack([e + 0.5, e * 2], 1)]
    pay_d = [torch.as_tensor(p, device=DEV) for p in pay]
    for removed in (0, 1):
        for pattern in PATTERNS:
            ii, jj, kk, want = prune_edges(E, pattern, removed, rng)
            keep, ii2, jj2, kk2 = ku.np_prune(ii, jj, kk, removed, K, N_FR, M, WINDOW)
            assert np.array_equal(keep, want), (pattern, removed)   # the pattern is what the masks give
            idx_d = [torch.as_tensor(a, device=DEV) for a in (ii, jj, kk)]
            ins = idx_d + pay_d
            ins_before = [t.clone() for t in ins]
            outs = [torch.full((E + 2 * pad, *t.shape[1:]), CANARY, dtype=t.dtype, device=DEV) for t in ins]
            ws = workspace(E, removed)
            ptr = lambda t: t.data_ptr() if t.numel() else None
            rc = L.bt_edges_prune(K, N_FR, M, WINDOW, *(ptr(t) for t in ins), E, *(o[pad:].data_ptr() for o in outs), ws.data_ptr(), stream())
            assert rc == _lib.BT_OK
            s = status(ws)
            Eo = int(keep.sum())
            assert s.E_out == Eo and s.removed == removed, (pattern, removed, s.E_out, Eo)
            assert ws[2:4].tolist() == [0x5A5A5A5A5A5A5A5A] * 2      # the magnitudes and counts are not this stage's
            for o, ref in zip(outs, (ii2, jj2, kk2, pay[0][keep], pay[1][keep], pay[2][keep])):
                o = o.cpu().numpy()
                assert np.array_equal(o[pad:pad + Eo], ref.reshape(Eo, *o.shape[1:])), (pattern, removed)
                assert (o[:pad] == CANARY).all() and (o[pad + Eo:] == CANARY).all(), (pattern, removed)   # rows >= E_out and around
            assert all(torch.equal(a, b) for a, b in zip(ins, ins_before))


def decide_scene(seed=3, N=16, Mp=8):
    rng = np.random.default_rng(seed)
    s = np.arange(N)[:, None]
    xi = s * 0.06 * np.array([0.5, 0.1, 1.0, 0.0, 0.1, 0.02]) + np.sin(s * 0.7) * np.array([0.0, 0.04, 0.0, 0.01, 0.0, 0.02])
    poses = graphgen.se3_exp(xi).astype(np.float32)
    Kc = (np.tile(np.array([320.0, 310.0, 160.0, 120.0]), (N, 1)) * rng.uniform(0.95, 1.05, (N, 4))).astype(np.float32)
    pat = np.stack([rng.uniform(10, 310, N * Mp), rng.uniform(10, 230, N * Mp), rng.uniform(0.2, 1.0, N * Mp)], 1).astype(np.float32)
    return poses, Kc, pat.reshape(N * Mp, 3, 1, 1)


def decide_edges(E, sel_pos, k, rng, N=16, Mp=8):
    """E edges none of which is selected, then the positions `sel_pos` turned into (k-1 -> k) and (k+1 -> k) alternately."""
    ii = rng.integers(0, N, E)
    jj = rng.integers(0, N, E)
    jj[(jj == k) & ((ii == k - 1) | (ii == k + 1))] = k + 2
    sel_pos = np.asarray(sel_pos, dtype=np.int64)
    ii[sel_pos] = np.where(np.arange(sel_pos.size) % 2 == 0, k - 1, k + 1)
    jj[sel_pos] = k
    kk = ii * Mp + rng.integers(0, Mp, E)
    return ii.astype(np.int64), jj.astype(np.int64), kk.astype(np.int64)


def run_decide(k, ii, jj, kk, poses, Kc, pat, thresh, ws=None, beta=0.5):
    up = lambda a: torch.as_tensor(a, device=DEV)
    t = [up(a) for a in (ii, jj, kk, poses, pat, Kc)]
    ws = workspace(ii.size) if ws is None else ws
    ptr = lambda x: x.data_ptr() if x.numel() else None
    rc = lib().bt_keyframe_decide(k, ptr(t[0]), ptr(t[1]), ptr(t[2]), ii.size, t[3].data_ptr(), poses.shape[0], t[4].data_ptr(),
                                  pat.shape[0], 1, t[5].data_ptr(), beta, thresh, ws.data_ptr(), stream())
    assert rc == _lib.BT_OK
    return status(ws), ws


DECIDE_CASES = {                        # name: (E, positions of the selected edges)
    "none": (300, []),
    "one_each": (300, [7, 211]),
    "64_each": (1000, list(range(100, 228))),
    "65_each": (1000, list(range(3, 1000, 7))[:130]),
    "several_workgroups": (5000, list(range(0, 5000, 3))),
    "last_partial_wave": (256 * 3 + 37, list(range(256 * 3, 256 * 3 + 37))),
    "more_than_the_grid": (256 * 256 + 700, list(range(0, 256 * 256 + 700, 11))),   # the grid-stride loop takes a second round
}


@pytest.mark.parametrize("name", sorted(DECIDE_CASES))
def test_decide_against_float64(name):
    E, sel = DECIDE_CASES[name]
    k = 9
    rng = np.random.default_rng(E)
    poses, Kc, pat = decide_scene()
    ii, jj, kk = decide_edges(E, sel, k, rng)
    want = [ku.mean_flow64(poses, pat, Kc, ii, jj, kk, i, k) for i in (k - 1, k + 1)]
    cnt = [int(((ii == i) & (jj == k)).sum()) for i in (k - 1, k + 1)]
    s, ws = run_decide(k, ii, jj, kk, poses, Kc, pat, 1e9)
    assert [s.cnt_prev, s.cnt_next] == cnt and ws[1].item() == 0x5A5A5A5A5A5A5A5A        # E_out is not this stage's
    if not sel:
        assert np.isnan(s.mag_prev) and np.isnan(s.mag_next) and s.removed == 0
        return
    for g, w in zip((s.mag_prev, s.mag_next), want):
        print(f"{name}: float64 {w!r} kernel {g!r} |difference| {abs(g - w):.3e} px")
        assert abs(g - w) <= MAG_TOL_PX
    half = (want[0] + want[1]) / 2
    assert s.removed == 1
    for thresh, removed in ((half + 0.5, 1), (half - 0.5, 0)):            # 0.5 px on either side: no summation order flips it
        s2, ws2 = run_decide(k, ii, jj, kk, poses, Kc, pat, thresh)
        assert s2.removed == removed
        assert ws2[2:4].cpu().numpy().tobytes() == ws[2:4].cpu().numpy().tobytes()     # a call repeats bit for bit


def test_decide_out_of_range_index_is_nan_and_kept():
    k = 9
    rng = np.random.default_rng(5)
    poses, Kc, pat = decide_scene()
    ii, jj, kk = decide_edges(400, list(range(50, 90)), k, rng)
    kk[51] = pat.shape[0]                                               # a (k+1 -> k) edge that names a patch past the buffer
    s, _ = run_decide(k, ii, jj, kk, poses, Kc, pat, 1e9)
    assert np.isnan(s.mag_next) and not np.isnan(s.mag_prev) and s.removed == 0 and s.cnt_next == 20
    kk[52] = -1                                                         # and a (k-1 -> k) one below it
    s, _ = run_decide(k, ii, jj, kk, poses, Kc, pat, 1e9)
    assert np.isnan(s.mag_next) and np.isnan(s.mag_prev) and s.removed == 0


def test_decide_without_candidate_reads_nothing():
    s, ws = run_decide(-1, *(np.zeros(0, np.int64),) * 3, *decide_scene(), 1e9)
    assert s.removed == 0 and np.isnan(s.mag_prev) and np.isnan(s.mag_next) and s.cnt_prev == s.cnt_next == 0
    ws = workspace(100, removed=1)
    rc = lib().bt_keyframe_decide(-1, None, None, None, 100, None, 0, None, 0, 0, None, 0.5, 1e9, ws.data_ptr(), stream())
    assert rc == _lib.BT_OK and status(ws).removed == 0


ROW_BYTES = (1, 3, 4, 8, 12, 4 * 5 + 2, 8 * 11 * 3 * 4)              # ..., 4 j + 2, M * S_local * 3 * 4 of the fixture's shapes


@pytest.mark.parametrize("moves", [0, 1, 3, 17])
@pytest.mark.parametrize("removed", [1, 0])
def test_rows_shift(moves, removed):
    k = 6
    n = k + 1 + moves
    rows, pad = n + 3, 64
    rng = np.random.default_rng(moves)
    specs = [(rb, 0) for rb in ROW_BYTES] + [(8, 1), (12, 2), (4, 3), (22, 1)]          # (row bytes, offset of the base pointer)
    host, dev, desc = [], [], (_lib.RowBuffer * len(specs))()
    for b, (rb, off) in enumerate(specs):
        a = rng.integers(0, 256, pad + off + rows * rb + pad).astype(np.uint8)
        host.append(a)
        dev.append(torch.as_tensor(a, device=DEV))
        desc[b] = _lib.RowBuffer(dev[b].data_ptr() + pad + off, rb)
    ws = workspace(0, removed)
    assert lib().bt_rows_shift(desc, len(specs), k, n, ws.data_ptr(), stream()) == _lib.BT_OK
    torch.cuda.synchronize()
    for (rb, off), a, d in zip(specs, host, dev):
        want = a.copy()
        body = want[pad + off:pad + off + rows * rb].reshape(rows, rb)               # a view: rows < k, row n-1, the rows past n and the pads stay
        if removed:
            body[k:n - 1] = body[k + 1:n].copy()
        assert np.array_equal(d.cpu().numpy(), want), (rb, off)
    assert ws[0].item() == removed and ws[1:4].tolist() == [0x5A5A5A5A5A5A5A5A] * 3   # the status is only read
