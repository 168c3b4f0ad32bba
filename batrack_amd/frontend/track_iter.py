"""The tracker's refinement iteration around its two update transformers (the reference's
main/frontend/md_tracker.py:181-413, `MDTracker.forward_iteration`, and :49-61, `sample_pos_embed`), HIP underneath
(batrack_amd/csrc/track_iter.hip through include/batrack_track.h, which holds the specification).

    sample_pos_embed(grid_size, embed_dim, coords [B,S,N,>=2]) -> [B, E, N]      the reference's signature and return
    build_tokens(coords [S,N,3], coords_sub | None, fcorrs [S,N,LRR], ffeats [S,N,C], track_mask [S,N], vis [S,N],
                 pos [N,E], time [S,E], w_flow [F,195], b_flow [F], fix_track_mask) -> x [N,S,E]           one launch
    apply_delta(delta [N,S,3+C], gamma, beta, w_u, b_u, state [S,N,3], ffeats [S,N,C], stride, Dz, d_range, d_near,
                use_log_depth, total=None, dyn_mask=None) -> out [S,N,3]; state and ffeats updated in place     one launch
    forward_iteration(self, fmaps, dmaps, coords_init, ...)      the loop in our own words, the reference's signature and
                                                                 return tuple; the transformers, `vis_predictor` and
                                                                 `motion_label_block` are called as the torch modules they are

Inference only (inputs are detached, no autograd through the kernels), GPU tensors only; no CPU fallback.  B = 1.

`install()` makes the reference's tracker use `sample_pos_embed` and `forward_iteration` from here."""
import importlib

import numpy as np
import torch

from .. import _lib
from .corr import CorrBlock

EMB = 195                    # BT_TRACK_EMB: get_3d_embedding(flow, 64) with the flow appended


def _gpu(name, t, what="track_iter"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: `{name}` must be a tensor on the GPU (there is no CPU fallback in batrack_amd)")
    return t.detach().float()


def _sincos_1d(dim, positions):
    """[len(positions), dim] = [sin(p w) | cos(p w)], w_i = 10000^(-i / (dim/2)), in float64 (embeddings.py:45-63)."""
    assert dim % 2 == 0
    omega = 1.0 / 10000 ** (np.arange(dim // 2, dtype=np.float64) / (dim / 2.0))
    out = np.einsum("m,d->md", np.asarray(positions, np.float64).reshape(-1), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


_tables = {}


def pos_tables(H, W, E, device):
    """The two 1-D tables of the separable 2-D sin-cos table: tabx [W, E/2], taby [H, E/2], float64 rounded to float32,
    built once per (H, W, E) and device."""
    key = (int(H), int(W), int(E), str(device))
    if key not in _tables:
        if E % 4:
            raise ValueError("track_iter: the embedding dimension must be a multiple of 4")
        f = lambda n: torch.from_numpy(_sincos_1d(E // 2, np.arange(n, dtype=np.float32)).astype(np.float32)).to(device)
        _tables[key] = (f(W), f(H))
    return _tables[key]


def time_table(S, E, device):
    key = ("t", int(S), int(E), str(device))
    if key not in _tables:
        _tables[key] = torch.from_numpy(_sincos_1d(E, np.arange(S, dtype=np.float32)).astype(np.float32)).to(device)
    return _tables[key]


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def pos_embed_rows(H, W, E, xy):
    """xy [N, >= 2] (unit last stride; a row view of the [S, N, 3] state is read in place) -> [N, E]."""
    xy = _gpu("coords", xy, "sample_pos_embed")
    assert xy.dim() == 2 and xy.shape[1] >= 2
    if xy.stride(1) != 1 or (xy.shape[0] > 1 and xy.stride(0) < 2):
        xy = xy.contiguous()
    tabx, taby = pos_tables(H, W, E, xy.device)
    ops = _lib.torch_ops()
    if ops is not None:
        return ops.track_pos_embed(tabx, taby, xy)
    N = xy.shape[0]
    out = torch.empty(N, E, dtype=torch.float32, device=xy.device)
    if N:
        _lib.check(_lib.lib().bt_track_pos_embed(tabx.data_ptr(), taby.data_ptr(), H, W, E, xy.data_ptr(), xy.stride(0) if N > 1 else 2,
                                                 N, out.data_ptr(), _stream(xy)), "bt_track_pos_embed")
    return out


def sample_pos_embed(grid_size, embed_dim, coords):
    coords = _gpu("coords", coords, "sample_pos_embed")
    B = coords.shape[0]
    assert B == 1 and coords.dim() == 4
    return pos_embed_rows(int(grid_size[0]), int(grid_size[1]), int(embed_dim), coords[0, 0]).t().unsqueeze(0)


def build_tokens(coords, coords_sub, fcorrs, ffeats, track_mask, vis, pos, time, w_flow, b_flow, fix_track_mask):
    c = lambda n, t: _gpu(n, t, "build_tokens").contiguous()
    coords, fcorrs, ffeats, track_mask, vis = c("coords", coords), c("fcorrs", fcorrs), c("ffeats", ffeats), c("track_mask", track_mask), c("vis", vis)
    pos, time, w_flow, b_flow = c("pos", pos), c("time", time), c("w_flow", w_flow), c("b_flow", b_flow)
    coords_sub = None if coords_sub is None else c("coords_sub", coords_sub)
    ops = _lib.torch_ops()
    if ops is not None:
        return ops.track_tokens(coords, coords_sub, fcorrs, ffeats, track_mask, vis, pos, time, w_flow, b_flow, bool(fix_track_mask))
    S, N, D = coords.shape
    LRR, C, F = fcorrs.shape[2], ffeats.shape[2], w_flow.shape[0]
    E = F + LRR + C + 2
    assert D == 3 and fcorrs.shape[:2] == (S, N) and ffeats.shape[:2] == (S, N) and track_mask.numel() == S * N and vis.numel() == S * N
    assert pos.numel() == N * E and time.numel() == S * E and w_flow.shape[1] == EMB and b_flow.numel() == F
    assert coords_sub is None or coords_sub.shape == coords.shape
    x = torch.empty(N, S, E, dtype=torch.float32, device=coords.device)
    if N:
        _lib.check(_lib.lib().bt_track_tokens(coords.data_ptr(), None if coords_sub is None else coords_sub.data_ptr(), fcorrs.data_ptr(),
                                              ffeats.data_ptr(), track_mask.data_ptr(), vis.data_ptr(), pos.data_ptr(), time.data_ptr(),
                                              w_flow.data_ptr(), b_flow.data_ptr(), S, N, F, LRR, C, int(bool(fix_track_mask)),
                                              x.data_ptr(), _stream(coords)), "bt_track_tokens")
    return x


def apply_delta(delta, gamma, beta, w_u, b_u, state, ffeats, stride, Dz, d_range, d_near, use_log_depth=False, total=None, dyn_mask=None):
    """`state` [S,N,3] and `ffeats` [S,N,C] must be contiguous float32 GPU tensors: they are updated in place."""
    c = lambda n, t: _gpu(n, t, "apply_delta").contiguous()
    delta, gamma, beta, w_u, b_u = c("delta", delta), c("gamma", gamma), c("beta", beta), c("w_u", w_u), c("b_u", b_u)
    for n, t in (("state", state), ("ffeats", ffeats)):
        if _gpu(n, t, "apply_delta").data_ptr() != t.data_ptr() or not t.is_contiguous():
            raise RuntimeError(f"apply_delta: `{n}` is updated in place: it must be a contiguous float32 tensor")
    if (total is None) != (dyn_mask is None):
        raise RuntimeError("apply_delta: `total` and `dyn_mask` come together (the static pass)")
    if total is not None:
        total, dyn_mask = c("total", total), c("dyn_mask", dyn_mask)
    ops = _lib.torch_ops()
    if ops is not None:
        return ops.track_apply(delta, gamma, beta, w_u, b_u, state.detach(), ffeats.detach(), total, dyn_mask, float(stride), float(Dz),
                               float(d_range), float(d_near), bool(use_log_depth))
    N, S, D = delta.shape
    C = D - 3
    assert state.shape == (S, N, 3) and ffeats.shape == (S, N, C) and gamma.numel() == C and beta.numel() == C
    assert w_u.numel() == C * C and b_u.numel() == C and (total is None or (total.shape == state.shape and dyn_mask.numel() == N))
    out = torch.empty_like(state)
    if N:
        _lib.check(_lib.lib().bt_track_apply(delta.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w_u.data_ptr(), b_u.data_ptr(),
                                             state.data_ptr(), ffeats.data_ptr(), None if total is None else total.data_ptr(),
                                             None if total is None else dyn_mask.data_ptr(), S, N, C, float(stride), float(Dz),
                                             float(d_range), float(d_near), int(bool(use_log_depth)), out.data_ptr(), _stream(delta)),
                   "bt_track_apply")
    return out


def forward_iteration(self, fmaps, dmaps, coords_init, coords_dyn_init, feat_init=None, vis_init=None, track_mask=None, iters=4):
    B, S_init, N, D = coords_init.shape
    assert D == 3
    assert B == 1
    B, S, __, H8, W8 = fmaps.shape
    device = fmaps.device

    def own(t, frames):
        """[1, frames', N, k] -> our own contiguous float32 [frames, N, k], the last frame repeated up to `frames`."""
        t = _gpu("a state tensor", t, "forward_iteration")[0]
        if t.shape[0] < frames:
            t = torch.cat([t, t[-1:].expand(frames - t.shape[0], -1, -1)], 0)
        return t.contiguous().clone()

    coords, coords_dyn = own(coords_init, S), own(coords_dyn_init, S)
    vis = own(vis_init, S if S_init < S else vis_init.shape[1])[..., 0]
    tm = _gpu("track_mask", track_mask, "forward_iteration")[0, ..., 0]
    if tm.shape[0] < vis.shape[0]:
        tm = torch.cat([tm, tm.new_zeros(vis.shape[0] - tm.shape[0], N)], 0)
    tm = tm.contiguous()
    ffeats, ffeats_static = own(feat_init, feat_init.shape[1]), own(feat_init, feat_init.shape[1])

    fcorr_fn = CorrBlock(fmaps, num_levels=self.corr_levels, radius=self.corr_radius)
    E = self.input_dim
    pos = pos_embed_rows(H8, W8, E, coords[0])
    pos_static = pos_embed_rows(H8, W8, E, (coords - coords_dyn)[0])
    time = time_table(S, E, device)

    p32 = lambda t: t.detach().float().contiguous()
    w_flow, b_flow = p32(self.zeroMLPflow.weight), p32(self.zeroMLPflow.bias)
    gamma, beta = p32(self.norm.weight), p32(self.norm.bias)
    w_u, b_u = p32(self.ffeat_updater[0].weight), p32(self.ffeat_updater[0].bias)
    scale = dict(stride=float(self.stride), Dz=float(self.Dz), d_range=float(self.d_far - self.d_near), d_near=float(self.d_near),
                 use_log_depth=bool(getattr(self, "use_log_depth", False)))

    coord_predictions, coord_depth_predictions, coord_static_predictions = [], [], []
    for __ in range(iters):
        fcorr_fn.corr(ffeats[None])
        fcorrs = fcorr_fn.sample(coords[None][..., :2])[0]
        x = build_tokens(coords, None, fcorrs, ffeats, tm, vis, pos, time, w_flow, b_flow, self.fix_track_mask)
        delta = self.updateformer(x[None])
        out = apply_delta(delta[0], gamma, beta, w_u, b_u, coords, ffeats, **scale)[None]
        coord_predictions.append(out[..., :2])
        coord_depth_predictions.append(out[..., 2:])

    vis_e = self.vis_predictor(ffeats.reshape(S * N, -1)).reshape(B, S, N)
    if self.motion_label_block is not None:
        dynamic_e = self.motion_label_block(ffeats[None], coords[None]).squeeze(2)
    else:
        dynamic_e = torch.ones(B, N, device=device)
    dyn_mask = torch.sigmoid(dynamic_e.detach().float())[0].contiguous()

    for __ in range(self.static_iters):
        fcorr_fn.corr(ffeats_static[None])
        fcorrs = fcorr_fn.sample((coords - coords_dyn)[None][..., :2])[0]
        x = build_tokens(coords, coords_dyn, fcorrs, ffeats_static, tm, vis, pos_static, time, w_flow, b_flow, self.fix_track_mask)
        delta = self.updateformer_dyn(x[None])
        out = apply_delta(delta[0], gamma, beta, w_u, b_u, coords_dyn, ffeats_static, total=coords, dyn_mask=dyn_mask, **scale)[None]
        coord_static_predictions.append(out)

    return coord_predictions, coord_depth_predictions, coord_static_predictions, vis_e, dynamic_e, feat_init


def install(module=None):
    """Rebind `sample_pos_embed` in the reference's tracker module (`main.frontend.md_tracker`, or the module given) and set
    its `MDTracker.forward_iteration` to the functions above; returns what was bound before, as
    (sample_pos_embed, forward_iteration).  Opt-in: nothing in batrack_amd calls it."""
    if module is None:
        module = importlib.import_module("main.frontend.md_tracker")
    previous = (getattr(module, "sample_pos_embed", None), getattr(module.MDTracker, "forward_iteration", None))
    module.sample_pos_embed = sample_pos_embed
    module.MDTracker.forward_iteration = forward_iteration
    return previous
