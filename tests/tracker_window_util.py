"""Shared by the tracker-window tests, the fixture generator and the measurement tool: the fixture's cases and their seeded
inputs, the stand-ins the window loop is run with, and a torch restatement of include/batrack_window.h and of the window
loop in our own words — the CPU specification, and on the GPU the baseline (the torch-operation form the kernels replace).
Every function computes in the dtype of the tensors it is given."""
import os
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from track_iter_util import digest, floor_int32              # noqa: F401  (one copy of each)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracker_window.npz")

C, EMB, STRIDE = 128, 63, 4
F64_STEP = 32            # the float64 run's feature maps are stored every 32nd element

# A: three windows; new tracks join in the first two; two sliding halves (frame0 = 2); the last window is padded; the last
#    window has no new track.   B: 9 x 18 maps (162 pixels: no multiple of 16 or 64).   C: the single-window call.
# Queries run from 3 px outside the image to 3 px outside on the far side: the feature sample clamps.
CASES = dict(A=dict(seed=61, S=4, T=7, H=20, W=28, first=(0, 0, 1, 3, 4, 5, 2)),
             B=dict(seed=62, S=2, T=3, H=36, W=72, first=(0, 1, 2)),
             C=dict(seed=63, S=4, T=4, H=20, W=28, first=(0, 3)))
INPUTS = ("rgbds", "queries", "conv_w", "conv_b")
WINDOW_KEYS = ("dmaps", "feat_init", "coords_init", "coords_dyn_init", "vis_init", "track_mask")
RETURNS = ("traj_e", "feat_init", "depth_e", "traj_static_e", "vis_e", "dynamic_e")


def make_inputs(seed, T, H, W, first, **_):
    """Seeded inputs of one case: float32 values in float64 arrays."""
    rng = np.random.default_rng(seed)
    N = len(first)
    rgbds = np.concatenate([rng.integers(0, 256, (1, T, 3, H, W)).astype(np.float64), rng.uniform(0.5, 20.0, (1, T, 1, H, W))], 2)
    rgbds[0, :, 3, 0, 0] = 0.0                                # below the 0.01 mask: not part of the range
    x = np.linspace(-3.0, W + 3.0, N) if N > 1 else np.array([W / 2.0])
    y = np.linspace(H + 3.0, -3.0, N) if N > 1 else np.array([H / 2.0])
    queries = np.stack([np.asarray(first, np.float64), x + rng.uniform(-0.4, 0.4, N), y + rng.uniform(-0.4, 0.4, N),
                        rng.uniform(0.5, 20.0, N)], -1)[None]
    k = 1 / np.sqrt((C + EMB) * 9)
    d = dict(rgbds=rgbds, queries=queries, conv_w=rng.uniform(-k, k, (C, C + EMB, 3, 3)) * 4, conv_b=rng.uniform(-0.5, 0.5, C))
    return {k: v.astype(np.float32).astype(np.float64) for k, v in d.items()}


def fnet_maps(seed, call, frames, h, w):
    """What the stand-in encoder returns on its call number `call` for `frames` frames (float32 values)."""
    rng = np.random.default_rng(1000 * seed + call)
    return rng.standard_normal((frames, C, h, w)).astype(np.float32)


def iteration_outputs(seed, call, S, n):
    """What the stand-in `forward_iteration` returns on its call number `call` for n tracks (float32 values)."""
    rng = np.random.default_rng(1000 * seed + 500 + call)
    f = lambda a: a.astype(np.float32)
    return dict(coords=f(rng.uniform(-4, 40, (1, S, n, 2))), coords_depth=f(rng.uniform(0.5, 20, (1, S, n, 1))),
                coords_static_3d=f(np.concatenate([rng.uniform(-4, 40, (1, S, n, 2)), rng.uniform(0.5, 20, (1, S, n, 1))], -1)),
                vis=f(rng.uniform(-6, 6, (1, S, n))), dynamic=f(rng.uniform(-4, 4, (1, n))))


class StandIn:
    """The plain object `forward` is run on, unbound: the attributes it reads, a stand-in encoder that returns seeded maps
    and a stand-in `forward_iteration` that records what it is given (`seen`) and returns prepared, seeded outputs.
    `embedConv` is a real Conv2d with the case's weights and (non-zero) bias; `embed3d` is whatever the caller supplies with
    a `freq_bands` list (the reference's Embedder_Fourier in the generator)."""

    def __init__(self, case, dtype, device, embed3d, log=False):
        spec = CASES[case]
        d = make_inputs(**spec)
        self.spec, self.dtype, self.device = spec, dtype, device
        self.S, self.stride, self.latent_dim, self.Embed3D, self.use_log_depth = spec["S"], STRIDE, C, True, log
        self.depth_drop_rate = 0.0
        self.embed3d = embed3d
        conv = nn.Conv2d(C + EMB, C, 3, padding=1).to(dtype)
        conv.weight.data.copy_(torch.as_tensor(d["conv_w"], dtype=dtype))
        conv.bias.data.copy_(torch.as_tensor(d["conv_b"], dtype=dtype))
        self.embedConv = conv.to(device).requires_grad_(False)
        self.seen, self.fnet_calls, self.fnet_out = [], 0, []

    def depth_process(self, depth_raw):
        return torch.log(depth_raw.clamp(min=1e-3)) if self.use_log_depth else depth_raw

    def fnet(self, rgbs):
        h, w = rgbs.shape[-2] // STRIDE, rgbs.shape[-1] // STRIDE
        out = torch.as_tensor(fnet_maps(self.spec["seed"], self.fnet_calls, rgbs.shape[0], h, w), dtype=self.dtype, device=self.device)
        self.fnet_calls += 1
        self.fnet_out.append(out)
        return out

    def forward_iteration(self, fmaps, dmaps, coords_init, coords_dyn_init, feat_init=None, vis_init=None, track_mask=None, iters=4):
        given = dict(fmaps=fmaps, dmaps=dmaps, coords_init=coords_init, coords_dyn_init=coords_dyn_init, feat_init=feat_init,
                     vis_init=vis_init, track_mask=track_mask)
        self.seen.append({k: v.detach().clone() for k, v in given.items()})
        o = iteration_outputs(self.spec["seed"], len(self.seen) - 1, self.S, coords_init.shape[2])
        t = lambda a: torch.as_tensor(a, dtype=self.dtype, device=self.device)
        return [t(o["coords"])], [t(o["coords_depth"])], [t(o["coords_static_3d"])], t(o["vis"]), t(o["dynamic"]), feat_init


def case_tensors(case, dtype=torch.float32, device="cpu"):
    d = make_inputs(**CASES[case])
    return {k: torch.as_tensor(v, dtype=dtype, device=device) for k, v in d.items()}


def computed_frames(window, S):
    """Which frames of a window's feature maps the window computed: all of the first, the new half of a slide."""
    return slice(0, S) if window == 0 else slice(S // 2, S)


# ------------------------------------------------------------------------------------------------------ the restatement
FREQS = [float(f) for f in (2.0 ** torch.linspace(0.0, 10.0, 10)).numpy().tolist()]       # Embedder_Fourier(max_freq_log2=10, N_freqs=10)


def depth_process(d, log):
    return torch.log(d.clamp(min=1e-3)) if log else d


def depth_range(depth, log):
    v = depth_process(depth, log)
    if not log:
        v = v[v > 0.01]
    return float(v.min()), float(v.max())


def window_depth(depth, S, stride, d_near, d_far, Dz, log):
    """depth [frames <= S, H, W] -> dmaps [S, h, w] (the last frame repeated), and their (min, max) as 0-dim tensors."""
    if depth.shape[0] < S:
        depth = torch.cat([depth, depth[-1:].expand(S - depth.shape[0], -1, -1)], 0)
    h, w = depth.shape[1] // stride, depth.shape[2] // stride
    d = depth_process(depth[:, ::stride, ::stride][:, :h, :w], log)
    div = torch.tensor(d_far - d_near, dtype=d.dtype, device=d.device)       # a tensor divisor: a true division on every device
    dm = ((d - d_near) / div) * Dz
    return dm, (dm.min(), dm.max())


def embedding(dmaps, zrange, freqs=FREQS):
    """dmaps [S, h, w] -> the 63 embedding channels [S, 63, h, w]: the normalised (x, y, z), then per frequency sin and cos."""
    S, h, w = dmaps.shape
    t = lambda v: torch.tensor(float(v), dtype=dmaps.dtype, device=dmaps.device)
    nm = lambda v, lo, hi: 2 * ((v - lo) / (hi - lo) - 0.5)
    gx = torch.arange(w, dtype=dmaps.dtype, device=dmaps.device)[None, None, :].expand(S, h, w)
    gy = torch.arange(h, dtype=dmaps.dtype, device=dmaps.device)[None, :, None].expand(S, h, w)
    p = torch.stack([nm(gx, t(0), t(w - 1)), nm(gy, t(0), t(h - 1)), nm(dmaps, zrange[0], zrange[1])], 1)
    out = [p]
    for f in freqs:
        out += [torch.sin(p * f), torch.cos(p * f)]
    return torch.cat(out, 1)


def embed_conv(fnet, dmaps, zrange, frame0, weight, bias, freqs=FREQS):
    F = fnet.shape[0]
    pe = embedding(dmaps, zrange, freqs)[frame0:frame0 + F]
    return Fn.conv2d(torch.cat([fnet, pe], 1), weight, bias, padding=1)


def sample_features(fmaps, frames, xy):
    """fmaps [S, C, h, w], frames [n], xy [n, >= 2] -> [n, C]: bilinear_sample2d on each query's own frame.  The reference
    takes the coordinates and the weights in float32 whatever the maps' dtype is (model_utils.py:84-85), and so does this."""
    S, __, h, w = fmaps.shape
    x, y = xy[:, 0].float(), xy[:, 1].float()
    x0, y0 = floor_int32(x), floor_int32(y)
    x1, y1 = x0 + 1, y0 + 1
    ix = lambda v, hi: v.clamp(0, hi).long()
    fr = frames.long().clamp(0, S - 1)
    tap = lambda yy, xx: fmaps[fr, :, ix(yy, h - 1), ix(xx, w - 1)]
    w00, w01, w10, w11 = ((x1 - x) * (y1 - y))[:, None], ((x - x0) * (y1 - y))[:, None], ((x1 - x) * (y - y0))[:, None], ((x - x0) * (y - y0))[:, None]
    return w00 * tap(y0, x0) + w01 * tap(y0, x1) + w10 * tap(y1, x0) + w11 * tap(y1, x1)


def pack_weights(weight):
    """The repack stated element by element: packed[c // 8, 3 ky + kx, c % 8, o] = weight[o, c, ky, kx]."""
    out = torch.zeros(24, 9, 8, C, dtype=weight.dtype)
    for c in range(C + EMB):
        out[c // 8, :, c % 8, :] = weight[:, c].reshape(C, 9).t()
    return out


# ------------------------------------------------------------------------------------- one-hot convolutions (the limits suite)
ONE_HOT_CONVS = 14           # 14 x 128 = 1792 output channels for the 191 x 9 = 1719 (channel, tap) pairs: 73 pairs come twice


def one_hot_taps(seed=83):
    """[14, 128, 3] int64: the (c, ky, kx) whose weight is 1 for each output channel of each convolution.  Every pair of an
    input channel and a tap occurs once, 73 drawn ones a second time, assigned to the output channels in a seeded shuffle."""
    g = torch.Generator().manual_seed(seed)
    pairs = (C + EMB) * 9
    every = torch.cat([torch.arange(pairs), torch.randint(0, pairs, (ONE_HOT_CONVS * C - pairs,), generator=g)])
    every = every[torch.randperm(every.numel(), generator=g)]
    return torch.stack([every // 9, (every % 9) // 3, every % 3], -1).reshape(ONE_HOT_CONVS, C, 3)


def one_hot_weight(taps, dtype=torch.float32):
    """taps [128, 3] -> the weight [128, 191, 3, 3] that is zero except W[o, c(o), ky(o), kx(o)] = 1."""
    w = torch.zeros(C, C + EMB, 3, 3, dtype=dtype)
    w[torch.arange(C), taps[:, 0], taps[:, 1], taps[:, 2]] = 1
    return w


def one_hot_select(inp, taps):
    """inp [F, 191 or fewer, h, w], taps [k, 3] -> [F, k, h, w]: in[f, c(o), y + ky(o) - 1, x + kx(o) - 1], zero outside the
    map — what a one-hot convolution leaves of its input before the bias, by padding and slicing."""
    h, w = inp.shape[-2:]
    padded = Fn.pad(inp, (1, 1, 1, 1))
    return torch.stack([padded[:, c, ky:ky + h, kx:kx + w] for c, ky, kx in taps.tolist()], 1)


def forward(me, rgbds, queries, iters=4):
    """The window loop on a StandIn, in the dtype of `rgbds`; returns the reference's tuple.  rgbds is normalised in place."""
    dt, dev = rgbds.dtype, rgbds.device
    B, T, __, H, W = rgbds.shape
    N, S, stride, half, log = queries.shape[1], me.S, me.stride, me.S // 2, me.use_log_depth
    div = lambda a, b: a / torch.tensor(b, dtype=dt, device=dev)
    first = queries[0, :, 0].long()
    __, order = torch.sort(first, dim=0, stable=True)
    inv = torch.argsort(order)
    first_s = first[order]
    rgbds[:, :, :3] = 2 * div(rgbds[:, :, :3], 255.0) - 1.0
    d_near, d_far = depth_range(rgbds[0, :, 3], log)
    me.d_near, me.d_far, me.Dz = d_near, d_far, W // stride
    Dz, h, w = me.Dz, H // stride, W // stride
    znorm = lambda d: div(depth_process(d, log) - d_near, d_far - d_near) * Dz
    out = dict(traj_e=torch.zeros(B, T, N, 2, dtype=dt, device=dev), depth_e=torch.zeros(B, T, N, 1, dtype=dt, device=dev),
               traj_static_e=torch.zeros(B, T, N, 3, dtype=dt, device=dev), vis_e=torch.zeros(B, T, N, dtype=dt, device=dev),
               dynamic_e=torch.zeros(B, T, N, dtype=dt, device=dev))
    mask = (torch.arange(T, device=dev)[None, :, None] >= first_s[None, None, :])[..., None]
    q = queries[0, order, 1:]
    ci = torch.cat([q[:, :2] / stride, znorm(q[:, 2:])], -1)[None, None].repeat(1, S, 1, 1)
    cd, vi = torch.zeros_like(ci), torch.full((B, S, N, 1), 10.0, dtype=dt, device=dev)
    feat, fmaps_, prev, ind = None, None, 0, 0
    while ind < T - half:
        S_local = min(S, T - ind)
        rgbs = rgbds[0, ind:ind + S_local, :3]
        if S_local < S:
            rgbs = torch.cat([rgbs, rgbs[-1:].expand(S - S_local, -1, -1, -1)], 0)
        dm, zr = window_depth(rgbds[0, ind:ind + S_local, 3], S, stride, d_near, d_far, Dz, log)
        wgt, b = me.embedConv.weight, me.embedConv.bias
        if fmaps_ is None:
            fmaps_ = embed_conv(me.fnet(rgbs), dm, zr, 0, wgt, b, me.embed3d.freq_bands)
        else:
            fmaps_ = torch.cat([fmaps_[half:], embed_conv(me.fnet(rgbs[half:]), dm, zr, half, wgt, b, me.embed3d.freq_bands)], 0)
        n = int((first_s < ind + S).sum())
        if n == 0:
            ind += half
            continue
        if n > prev:
            new = sample_features(fmaps_, first_s[prev:n] - ind, ci[0, 0, prev:n])
            new = new[None, None].repeat(1, S, 1, 1)
            feat = new if feat is None else torch.cat([feat, new], 2)
        if prev > 0:
            c2 = coords[-1][:, half:] / stride
            cz = znorm(coords_depth[-1][:, half:])
            nc = torch.cat([c2, cz], -1)
            ci[:, :half, :prev], ci[:, half:, :prev] = nc, nc[:, -1:].expand(-1, half, -1, -1)
            d2 = (c2 - static[-1][:, half:, :, :2]) / stride
            dz = znorm(cz - static[-1][:, half:, :, 2:])
            nd = torch.cat([d2, dz], -1)
            cd[:, :half, :prev], cd[:, half:, :prev] = nd, nd[:, -1:].expand(-1, half, -1, -1)
            nv = vis[:, half:, :, None]
            vi[:, :half, :prev], vi[:, half:, :prev] = nv, nv[:, -1:].expand(-1, half, -1, -1)
        coords, coords_depth, static, vis, dyn, __ = me.forward_iteration(
            fmaps=fmaps_[None], dmaps=dm[None, :, None], coords_init=ci[:, :, :n], coords_dyn_init=cd[:, :, :n], feat_init=feat[:, :, :n],
            vis_init=vi[:, :, :n], track_mask=mask[:, ind:ind + S, :n], iters=iters)
        out["traj_e"][:, ind:ind + S, :n] = coords[-1][:, :S_local]
        out["depth_e"][:, ind:ind + S, :n] = coords_depth[-1][:, :S_local]
        out["traj_static_e"][:, ind:ind + S, :n] = static[-1][:, :S_local]
        out["vis_e"][:, ind:ind + S, :n] = vis[:, :S_local]
        out["dynamic_e"][:, ind:ind + S, :n] = dyn[:, None]
        mask = mask.clone()
        mask[:, :ind + S, :n] = False
        ind, prev = ind + half, n
    o = {k: v[:, :, inv] for k, v in out.items()}
    return o["traj_e"], feat, o["depth_e"], o["traj_static_e"], torch.sigmoid(o["vis_e"]), torch.sigmoid(o["dynamic_e"]), None


def embed3d_stand_in():
    """An object with the `freq_bands` the reference's Embedder_Fourier(3, 10.0, 10) has."""
    return types.SimpleNamespace(freq_bands=list(FREQS))
