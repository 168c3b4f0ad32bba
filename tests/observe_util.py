"""The specification of bt_observe_window (include/batrack_observe.h) restated with torch tensor operations, float32,
every operation a rounded one: what tests/golden/observe_window.npz (made by the reference's unmodified predict_target)
is compared with on the CPU, what the GPU tests compare the kernel with, and — it has the signature of
batrack_amd.frontend.observe.window_observations — the `observer` of a WindowedBA on any device.

The threshold of the motion decoupling is taken as the reference takes it: on the host (two `.item()`s here)."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "observe_window.npz")
CASES = ("a", "b", "c_below", "c_above", "d_len", "d_init", "e")
BUFFERS = ("patches_local", "local_monodisp", "local_vis", "local_static", "local_weights")
OUTPUTS = ("targets_3d", "weights", "weights_pose", "query_disp", "patches_valid") + BUFFERS


def f32(x):
    """A Python number rounded to float32 once (how a tensor operation takes a Python scalar)."""
    return float(np.float32(x))


def quantile_threshold(values, q):
    """torch.quantile(values, q) with the default linear interpolation, for a float32 tensor of any shape, spelt out: the
    rank in float32, the two order statistics around it, torch.lerp on the CPU.  A NaN in `values` gives NaN.  Returns a
    float32 CPU scalar tensor."""
    v = values.detach().reshape(-1)
    if bool(torch.isnan(v).any()):
        return torch.tensor(float("nan"), dtype=torch.float32)
    srt = torch.sort(v).values
    rank = np.float32(q) * np.float32(v.numel() - 1)
    lo, hi = int(np.floor(rank)), int(np.ceil(rank))
    w = np.float32(rank - np.float32(lo))
    a, b = (torch.tensor(srt[k].item(), dtype=torch.float32) for k in (lo, hi))
    return torch.lerp(a, b, torch.tensor(w, dtype=torch.float32))


def static_threshold(dyn, static_quantile, static_thr):
    """min(quantile(1 - dyn, 1 - STATIC_QUANTILE), STATIC_THRESHOLD) as Python's min takes it (a NaN quantile stays), as the
    float32 number the comparison `static >= th` then uses."""
    th = quantile_threshold(1 - dyn, 1 - static_quantile).item()
    return f32(min(th, static_thr))


def floor_int32(v):
    """floor(v).int() as the reference's x86 host converts, held in float: a floor that does not fit an int32 (beyond 2^31 on
    either side, or NaN) is INT_MIN (the same as track_iter_util.floor_int32)."""
    f = torch.floor(v)
    return torch.where((f >= -2.0 ** 31) & (f < 2.0 ** 31), f, torch.full_like(f, -2.0 ** 31))


def sample_maps(dmaps, queries):
    """The depth maps [S', H, W] at the queries (t, x, y) [Nq, 3]: floor (converted to int32 as the reference's host does),
    clamped indices, weights from the unclamped corners, the four products summed left to right."""
    _, H, W = dmaps.shape
    t, x, y = queries[:, 0].long(), queries[:, 1], queries[:, 2]
    x0, y0 = floor_int32(x), floor_int32(y)
    x1, y1 = x0 + 1, y0 + 1
    cx0, cx1 = (c.clamp(0, W - 1).long() for c in (x0, x1))
    cy0, cy1 = (c.clamp(0, H - 1).long() for c in (y0, y1))
    i00, i01, i10, i11 = dmaps[t, cy0, cx0], dmaps[t, cy0, cx1], dmaps[t, cy1, cx0], dmaps[t, cy1, cx1]
    w00, w01, w10, w11 = (x1 - x) * (y1 - y), (x - x0) * (y1 - y), (x1 - x) * (y - y0), (x - x0) * (y - y0)
    return ((w00 * i00 + w01 * i01) + w10 * i10) + w11 * i11


def clamp_min(d, lo=1e-2):
    """max(d, lo) where a NaN stays NaN."""
    return torch.where(d < lo, torch.full_like(d, lo), d)


def window_observations_ref(traj, depth, vis, dyn, queries, dmaps, ii, jj, kk, *, patches_valid, patches_local, local_monodisp=None,
                            local_vis=None, local_static=None, local_weights=None, n, window, kf_stride, wd, ht, cfg=None,
                            is_initialized=False, interp_shape=(384, 512), image_size=None, padding=20, sampler=None):
    """batrack_amd.frontend.observe.window_observations in tensor operations (same arguments, same returns, the buffers
    updated in place).  sampler: another form of `sample_maps` (tools/gpu_observe_bench.py times a per-query loop)."""
    if cfg is None:
        from batrack_amd.frontend.observe import ObserveConfig
        cfg = ObserveConfig()
    S, Nq = traj.shape[1], traj.shape[2]
    Sp = int(window)
    xy = traj.reshape(S, Nq, 2).clone()
    vis = vis.reshape(S, Nq).clone()
    depth, dyn = depth.reshape(S, Nq), dyn.reshape(S, Nq)
    q = queries.reshape(Nq, 3)
    N, M = patches_valid.shape
    query_disp = None
    if dmaps is not None:
        H, W = dmaps.shape[-2:]
        query_disp = 1.0 / clamp_min((sampler or sample_maps)(dmaps.reshape(Sp, H, W), q))
    elif image_size is not None:
        H, W = image_size
    # 1. the tracker's tail
    if interp_shape is not None and Nq:
        ih, iw = interp_shape
        tq, ar = q[:, 0].long(), torch.arange(Nq, device=q.device)
        xy[tq, ar, 0] = q[:, 1] * f32(iw / W)
        xy[tq, ar, 1] = q[:, 2] * f32(ih / H)
        vis[tq, ar] = 1.0
        xy[..., 0] *= f32(W / iw)
        xy[..., 1] *= f32(H / ih)
    # 3. labels
    vis_label = vis > f32(cfg.VIS_THRESHOLD) if cfg.VIS_THRESHOLD is not None else torch.ones_like(vis, dtype=torch.bool)
    x, y = xy[..., 0], xy[..., 1]
    inside = (x >= f32(padding)) & (x < f32(wd - padding)) & (y >= f32(padding)) & (y < f32(ht - padding))
    vis_raw = vis_label & inside
    # 4. motion decoupling over all S frames
    if Nq:
        th = static_threshold(dyn, cfg.STATIC_QUANTILE, cfg.STATIC_THRESHOLD)
        static_label = (1 - dyn) >= torch.tensor(th, dtype=torch.float32, device=dyn.device)
    else:
        static_label = torch.zeros_like(vis_raw)
    xy, depth, vis_label, vis_raw, static_label = xy[:Sp], depth[:Sp], vis_label[:Sp], vis_raw[:Sp], static_label[:Sp]
    rows = slice(n - Sp, n, kf_stride)
    # 5. validity while initialised
    if is_initialized:
        patches_valid[rows] = ((patches_valid[rows].reshape(-1) != 0) | (vis_label.sum(0) > 3)).reshape(-1, M).float()
    # 6. targets and weights, track-major
    target = torch.cat([xy, (1.0 / clamp_min(depth))[..., None]], -1).permute(1, 0, 2).reshape(Nq * Sp, 3)
    w = vis_raw.clone()
    if n >= cfg.MIN_TRACK_LEN:
        long_enough = vis_raw.sum(0) >= cfg.MIN_TRACK_LEN
        patches_valid[rows] = long_enough.reshape(-1, M).float()
        w = w & long_enough[None]
    edge = lambda a: a.permute(1, 0).reshape(Nq * Sp)
    w_e, static_e, raw_e = edge(w).float(), edge(static_label), edge(vis_raw).float()
    weights = torch.stack([w_e, w_e], 1)
    # 7.
    weights_pose = weights * static_e[:, None].float()
    # 8. window buffers
    S_local = patches_local.shape[-2]
    slot = jj - ii + (S_local + 1) // 2 - 1
    ok = (slot >= 0) & (slot < S_local) & (kk >= 0) & (kk < N * M)
    c = (kk * S_local + slot)[ok]
    patches_local.view(-1, 3)[c] = target[ok]
    for buf, val in ((local_monodisp, target[:, 2]), (local_vis, raw_e), (local_static, static_e.float()), (local_weights, w_e)):
        if buf is not None:
            buf.view(-1)[c] = val[ok]
    return target[None], weights[None], weights_pose[None], query_disp


def window_edges(n, Sp, M, kf_stride, device="cpu"):
    """(ii, jj, kk) of the window's new edges, track-major (batrack.py:399-410, 189-204)."""
    lo = n - Sp
    kf = torch.arange(lo, n, kf_stride, device=device)
    kk = (kf[:, None] * M + torch.arange(M, device=device)[None]).reshape(-1).repeat_interleave(Sp)
    jj = torch.arange(lo, n, device=device).repeat(kf.numel() * M)
    return kk // M, jj, kk


def load_case(z, c, device="cpu"):
    """Fixture case `c` as (inputs for window_observations[_ref] with fresh copies of the in/out buffers, expected arrays)."""
    g = lambda k: z[f"{c}.{k}"]
    t = lambda a: torch.as_tensor(np.array(a), device=device)
    S, Nq = g("traj").shape[:2]
    Sp, n, M, kf = int(g("Sp")), int(g("n")), int(g("M")), int(g("kf_stride"))
    from batrack_amd.frontend.observe import ObserveConfig
    vt = float(g("VIS_THRESHOLD"))
    cfg = ObserveConfig(VIS_THRESHOLD=None if np.isnan(vt) else vt, STATIC_THRESHOLD=float(g("STATIC_THRESHOLD")),
                        STATIC_QUANTILE=float(g("STATIC_QUANTILE")), MIN_TRACK_LEN=int(g("MIN_TRACK_LEN")))
    args = [t(g("traj"))[None], t(g("depth"))[None, ..., None], t(g("vis"))[None], t(g("dyn"))[None], t(g("queries"))[None],
            t(z["dmaps"][:Sp]), t(g("ii")), t(g("jj")), t(g("kk"))]
    kw = dict(patches_valid=t(g("patches_valid_in")), n=n, window=Sp, kf_stride=kf, wd=int(g("wd")), ht=int(g("ht")), cfg=cfg,
              is_initialized=bool(g("is_initialized")), interp_shape=(384, 512))
    for b in BUFFERS:
        kw[b] = t(g(b + "_in"))
    return args, kw, {k: g(k + "_out") if k in BUFFERS or k == "patches_valid" else g(k) for k in OUTPUTS}


def results(out, kw):
    """What a call returned and left in its buffers, as numpy arrays under the names of OUTPUTS."""
    r = dict(zip(OUTPUTS[:4], (None if o is None else o.detach().cpu().numpy() for o in out)))
    r["targets_3d"], r["weights"], r["weights_pose"] = (r[k][0] for k in OUTPUTS[:3])
    for k in ("patches_valid",) + BUFFERS:
        r[k] = None if kw.get(k) is None else kw[k].detach().cpu().numpy()
    return r


def same_bits(a, b):
    """Bit-for-bit equality of two float32 arrays (NaN payloads included)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def random_inputs(seed, Nq, M, S, Sp, kf, device="cpu", H=52, W=64, S_local=None, N=None, n=None, cfg=None, init=True,
                  dyn=None, interp_shape=(384, 512), maps=True, padding=20):
    """Generated inputs of any shape as (args, kw) of window_observations[_ref]: tracks around the padded image's bounds,
    visibilities around the threshold, a few NaN depths and coordinates, queries in and around the maps, buffers that hold
    values the step cannot write.  dyn: the dynamic scores [S, Nq] (default: most tracks static, some moving)."""
    rng = np.random.default_rng(seed)
    assert Nq == -(-Sp // kf) * M
    n = Sp + 3 if n is None else n
    N = n + 2 if N is None else N
    S_local = 2 * S - 1 if S_local is None else S_local
    ih, iw = interp_shape if interp_shape is not None else (H, W)
    xy = np.stack([rng.uniform(padding - 6, W - padding + 6, (S, Nq)) * iw / W, rng.uniform(padding - 6, H - padding + 6, (S, Nq)) * ih / H], -1)
    depth = rng.uniform(0.005, 6.0, (S, Nq))
    vis = np.where(rng.random((S, Nq)) < 0.75, rng.uniform(0.9, 1.0, (S, Nq)), rng.uniform(0.0, 0.9, (S, Nq)))
    if dyn is None:
        dyn = np.where(rng.random((1, Nq)) < 0.7, rng.uniform(0.0, 0.3, (S, Nq)), rng.uniform(0.85, 1.0, (S, Nq)))
    for a in (depth, xy[..., 0], xy[..., 1]):
        a[rng.random((S, Nq)) < 0.01] = np.nan
    queries = np.stack([(np.arange(Nq) // M) * kf, rng.uniform(-2, W + 2, Nq), rng.uniform(-2, H + 2, Nq)], 1)
    yy, xx = np.mgrid[0:H, 0:W]
    dmaps = np.stack([2.5 + 1.5 * np.sin(0.21 * xx + 0.4 * s) * np.cos(0.17 * yy - 0.3 * s) for s in range(Sp)]) if Sp else np.zeros((0, H, W))
    t = lambda a, dt=np.float32: torch.as_tensor(np.asarray(a, dt), device=device)
    few = lambda base, shape: t(base + rng.integers(0, 8, shape) * 0.125)
    ii, jj, kk = window_edges(n, Sp, M, kf, device)
    args = [t(xy)[None], t(depth)[None, ..., None], t(vis)[None], t(dyn)[None], t(queries)[None], t(dmaps) if maps else None, ii, jj, kk]
    kw = dict(patches_valid=t(rng.random((N, M)) < 0.3), patches_local=few(-9.0, (N * M, S_local, 3)),
              local_monodisp=few(-5.0, (N * M, S_local)), local_vis=few(2.0, (N * M, S_local)), local_static=few(3.0, (N * M, S_local)),
              local_weights=few(4.0, (N * M, S_local)), n=n, window=Sp, kf_stride=kf, wd=W, ht=H, cfg=cfg, is_initialized=init,
              interp_shape=interp_shape, image_size=(H, W), padding=padding)
    return args, kw


def clone_call(args, kw):
    """Fresh copies of the in/out buffers of a call (the inputs are shared)."""
    return args, {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
