"""Shared by the tracker-iteration tests, the fixture generator and the measurement tool: the fixture's cases and their
seeded inputs, and a torch restatement of include/batrack_track.h in our own words — the CPU specification, and on the
GPU the baseline (the torch-operation form the kernels replace).  Every function computes in the dtype of the tensors it
is given (float32: the reference's float32 run operation for operation; float64: the gate's other side)."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_iter.npz")

F, LRR, C, EMB = 130, 196, 128, 195
E = F + LRR + C + 2                       # 456: the update transformers' input width
LEVELS, RADIUS = 4, 3                     # LRR = LEVELS * (2 RADIUS + 1)^2

# the fixture's cases.  S_init < S (a): the state comes with fewer frames than the maps and is padded with its last frame,
# and so is the track mask, with zeros.  (b) has first-frame coordinates outside the map (the position sample clamps) and
# the depth through exp.  16 x 24 is the smallest map on which the reference's 4-level correlation block is finite.
CASES = dict(a=dict(seed=51, S=3, S_init=2, N=5, fix=0, iters=2, static=2, H=16, W=24, log=0),
             b=dict(seed=52, S=12, S_init=12, N=6, fix=1, iters=1, static=1, H=16, W=24, log=1),
             c=dict(seed=53, S=2, S_init=2, N=65, fix=0, iters=1, static=0, H=16, W=24, log=0),
             d=dict(seed=54, S=1, S_init=1, N=1, fix=0, iters=1, static=0, H=16, W=24, log=0))
INPUTS = ("fmaps", "coords_init", "coords_dyn_init", "feat_init", "vis_init", "track_mask", "w_flow", "b_flow", "gamma", "beta",
          "w_u", "b_u", "deltas", "dyn_logit")


def make_inputs(seed, S, S_init, N, H, W, iters, static, log, **_):
    """Seeded inputs of one case, float32 values in float64 arrays, with the batch dimension the tracker uses.  `scale`
    holds the tracker's scalars (stride, Dz, d_near, d_far, use_log_depth)."""
    rng = np.random.default_rng(seed)
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s)
    d = {}
    d["fmaps"] = rng.standard_normal((1, S, C, H, W))
    start = np.stack([u(1, W - 2, N), u(1, H - 2, N), u(0, W, N)], -1)                      # [N, 3]
    if seed == CASES["b"]["seed"]:
        start[:3, :2] = [(-3.5, 4.25), (W + 2.25, H + 1.5), (5.5, -0.75)]                    # outside the map: the sample clamps
    d["coords_init"] = (start[None] + 1.5 * rng.standard_normal((S_init, N, 3)) * (np.arange(S_init) > 0)[:, None, None])[None]
    d["coords_dyn_init"] = 0.5 * rng.standard_normal((1, S_init, N, 3))
    d["feat_init"] = rng.standard_normal((1, S, N, C))
    d["vis_init"] = u(-5, 10, 1, S_init, N, 1)
    d["track_mask"] = (rng.random((1, S_init, N, 1)) < 0.7).astype(np.float64)
    k = 1 / np.sqrt(EMB)
    d["w_flow"], d["b_flow"] = u(-k, k, F, EMB), u(-k, k, F)
    d["gamma"], d["beta"] = 1 + 0.1 * rng.standard_normal(C), 0.1 * rng.standard_normal(C)
    k = 1 / np.sqrt(C)
    d["w_u"], d["b_u"] = u(-k, k, C, C), u(-k, k, C)
    deltas = rng.standard_normal((iters + static, 1, N, S, 3 + C))
    deltas[..., :3] *= 0.5
    d["deltas"] = deltas
    d["dyn_logit"] = rng.standard_normal((1, N, 1))
    d = {k: v.astype(np.float32).astype(np.float64) for k, v in d.items()}
    d["scale"] = dict(stride=4.0, Dz=float(W), d_near=-0.7 if log else 0.5, d_far=3.0 if log else 20.0, use_log_depth=bool(log))
    return d


def digest(a):
    """Three float64 sums that move when any element of the array does."""
    a = np.asarray(a, np.float64).ravel()
    return np.array([a.sum(), (a * a).sum(), (a * (np.arange(a.size) % 97)).sum()])


# --------------------------------------------------------------------------------------------------------- the tables
def sincos_1d(dim, n):
    """[n, dim] float64: [sin(p w) | cos(p w)] for p = 0 .. n-1, w_i = 10000^(-2i / dim)."""
    w = 1.0 / 10000 ** (np.arange(dim // 2, dtype=np.float64) / (dim / 2.0))     # this order: the float32 rounding hangs on it
    a = np.arange(n, dtype=np.float64)[:, None] * w[None]
    return np.concatenate([np.sin(a), np.cos(a)], 1)


def pos_tables(H, W, E=E):
    """tabx [W, E/2], taby [H, E/2] float32: the 2-D table is T[y, x] = [tabx[x] | taby[y]]."""
    return torch.from_numpy(sincos_1d(E // 2, W).astype(np.float32)), torch.from_numpy(sincos_1d(E // 2, H).astype(np.float32))


def time_table(S, E=E):
    return torch.from_numpy(sincos_1d(E, S).astype(np.float32))


def full_table(H, W, E=E):
    """The [H, W, E] table the separable form replaces, float64 on the host rounded to float32."""
    tx, ty = sincos_1d(E // 2, W), sincos_1d(E // 2, H)
    return torch.from_numpy(np.concatenate([np.broadcast_to(tx[None], (H, W, E // 2)), np.broadcast_to(ty[:, None], (H, W, E // 2))], -1)
                            .astype(np.float32))


def floor_int32(v):
    """floor(v).int() as the reference's x86 host converts, held in float: a floor that does not fit an int32 (beyond 2^31 on
    either side, or NaN) is INT_MIN.  (torch's own .int() is undefined there: it saturates on a GPU.)  The + 1 that follows
    may be done in float: from 2^24 up it rounds to even exactly as the conversion of the int32 sum does."""
    f = torch.floor(v)
    return torch.where((f >= -2.0 ** 31) & (f < 2.0 ** 31), f, torch.full_like(f, -2.0 ** 31))


def _corners(xy, H, W):
    x, y = xy[:, 0].float(), xy[:, 1].float()
    x0, y0 = floor_int32(x), floor_int32(y)
    x1, y1 = x0 + 1, y0 + 1
    idx = lambda v, hi: v.clamp(0, hi).long()
    w = [((x1 - x) * (y1 - y))[:, None], ((x - x0) * (y1 - y))[:, None], ((x1 - x) * (y - y0))[:, None], ((x - x0) * (y - y0))[:, None]]
    return idx(x0, W - 1), idx(x1, W - 1), idx(y0, H - 1), idx(y1, H - 1), w


def pos_embed(tabx, taby, xy):
    """Bilinear sample of the separable table at xy [N, 2] -> [N, E] float32: corners clamped, weights from the unclamped
    corners, the four rounded products summed left to right."""
    ix0, ix1, iy0, iy1, (w00, w01, w10, w11) = _corners(xy, taby.shape[0], tabx.shape[0])
    ox = w00 * tabx[ix0] + w01 * tabx[ix1] + w10 * tabx[ix0] + w11 * tabx[ix1]
    oy = w00 * taby[iy0] + w01 * taby[iy0] + w10 * taby[iy1] + w11 * taby[iy1]
    return torch.cat([ox, oy], 1)


def pos_embed_full_table(H, W, E, xy):
    """The parent formulation: the whole table built on the host, uploaded, sampled at xy [N, 2]."""
    tab = full_table(H, W, E).to(xy.device)
    ix0, ix1, iy0, iy1, (w00, w01, w10, w11) = _corners(xy, H, W)
    return w00 * tab[iy0, ix0] + w01 * tab[iy0, ix1] + w10 * tab[iy1, ix0] + w11 * tab[iy1, ix1]


# ---------------------------------------------------------------------------------------------------- far coordinates
FAR_GOLD = os.path.join(os.path.dirname(GOLD), "pos_embed_far.npz")
FAR_H, FAR_W, FAR_E = 16, 24, 8          # the fixture's map; E = 8 keeps the file to a few KB


def far_values(W=FAR_W):
    """The finite float32 coordinates of tests/golden/pos_embed_far.npz: inside the map, just outside it, around 2^24 (where
    x + 1 starts to round), at 2^31 (where an int32 floor ends) and far beyond, up to FLT_MAX."""
    fmax = float(np.finfo(np.float32).max)
    v = [0.0, 3.25, 7.5, 15.0, 22.75, -3.5, W + 2.25]
    for a in (2.0 ** 24 + 1, 2.0 ** 24 + 2, 2.0 ** 31, 3e9, 1e30, fmax):
        v += [a, -a]
    return torch.tensor(v, dtype=torch.float32)


def far_pairs(values):
    """[V * V, 2]: every (x, y) pair, x outer."""
    V = values.numel()
    return torch.stack([values[:, None].expand(V, V), values[None, :].expand(V, V)], -1).reshape(V * V, 2).contiguous()


# ------------------------------------------------------------------------------------------------------------- tokens
def flow_embedding(flow):
    """[..., 3] -> [..., 195]: per axis sin / cos interleaved over 32 frequencies d_k = 2k * 15.625 held in float32, then
    the flow itself."""
    d = torch.arange(0, 64, 2, dtype=torch.float32, device=flow.device) * (1000.0 / 64)
    arg = flow[..., None] * d
    pe = torch.stack([torch.sin(arg), torch.cos(arg)], -1).reshape(*flow.shape[:-1], 192)
    return torch.cat([pe, flow], -1)


def mask_columns(track_mask, vis, fix):
    """track_mask, vis [S, N] -> [N, S, 2].  fix: (mask, vis) of the token.  Otherwise the reference's concatenation along
    N followed by a reshape: the [2N, S] array [mask^T ; vis^T] read as [N, S, 2]."""
    S, N = track_mask.shape
    if fix:
        return torch.stack([track_mask, vis], -1).permute(1, 0, 2)
    return torch.cat([track_mask.t(), vis.t()], 0).reshape(N, S, 2)


def tokens(coords, coords_sub, fcorrs, ffeats, track_mask, vis, pos, time, w_flow, b_flow, fix):
    """x [N, S, E]; coords (and coords_sub) [S, N, 3], fcorrs [S, N, LRR], ffeats [S, N, C], track_mask / vis [S, N]."""
    c = coords if coords_sub is None else coords - coords_sub
    flow = (c - c[0:1]).permute(1, 0, 2)
    fl = flow_embedding(flow) @ w_flow.t() + b_flow
    x = torch.cat([fl, fcorrs.permute(1, 0, 2), ffeats.permute(1, 0, 2), mask_columns(track_mask, vis, fix)], -1)
    return (x + pos[:, None]) + time[None]


# -------------------------------------------------------------------------------------------------------------- apply
def apply(delta, gamma, beta, w_u, b_u, state, ffeats, stride, Dz, d_range, d_near, use_log_depth, total=None, dyn_mask=None):
    """delta [N, S, 3 + C] -> (state', ffeats', out), nothing in place."""
    N, S, D = delta.shape
    g = delta[..., 3:]
    mean, var = g.mean(-1, keepdim=True), g.var(-1, unbiased=False, keepdim=True)
    y = ((g - mean) / torch.sqrt(var + 1e-5) * gamma + beta) @ w_u.t() + b_u
    y = 0.5 * y * (1 + torch.erf(y / np.sqrt(2.0)))
    ffeats = ffeats + y.permute(1, 0, 2)
    state = state + delta[..., :3].permute(1, 0, 2)
    p = state if total is None else total - state * dyn_mask[None, :, None]
    z = (p[..., 2] / Dz) * d_range + d_near
    out = torch.cat([p[..., :2] * stride, (torch.exp(z) if use_log_depth else z)[..., None]], -1)
    return state, ffeats, out


def pad_frames(a, frames, zeros=False):
    """[1, S', N, k] -> [frames, N, k]: the last frame repeated (or zeros appended) up to `frames`."""
    a = a[0]
    if a.shape[0] < frames:
        tail = torch.zeros_like(a[-1:]) if zeros else a[-1:]
        a = torch.cat([a, tail.expand(frames - a.shape[0], -1, -1)], 0)
    return a


def case_tensors(c, dtype=torch.float32, device="cpu"):
    """The case's inputs as tensors in the layouts of the ABI (state padded to S frames): a dict, with `spec` and `scale`."""
    spec = CASES[c]
    d = make_inputs(**spec)
    t = lambda a: torch.as_tensor(a, dtype=dtype, device=device)
    S = spec["S"]
    out = dict(spec=spec, scale=d["scale"], fmaps=t(d["fmaps"]), coords=pad_frames(t(d["coords_init"]), S),
               coords_dyn=pad_frames(t(d["coords_dyn_init"]), S), ffeats=t(d["feat_init"])[0], vis=pad_frames(t(d["vis_init"]), S)[..., 0],
               track_mask=pad_frames(t(d["track_mask"]), S, zeros=True)[..., 0], deltas=t(d["deltas"])[:, 0], dyn_logit=t(d["dyn_logit"]))
    for k in ("w_flow", "b_flow", "gamma", "beta", "w_u", "b_u"):
        out[k] = t(d[k])
    return out


def scale_args(scale):
    return dict(stride=scale["stride"], Dz=scale["Dz"], d_range=scale["d_far"] - scale["d_near"], d_near=scale["d_near"],
                use_log_depth=scale["use_log_depth"])
