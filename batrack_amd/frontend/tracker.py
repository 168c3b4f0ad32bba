"""The tracker's window loop (the reference's main/frontend/md_tracker.py:416-671, `MDTracker.forward`): everything that
prepares the windows `forward_iteration` consumes, HIP underneath (batrack_amd/csrc/window_fmaps.hip through
include/batrack_window.h, which holds the specification).

    depth_range(depth [T,H,W], use_log_depth=False) -> [2] on the device         masked min / max of the video's depth, one launch
    window_depth(depth [frames<=S,H,W], S, stride, d_near, d_far, Dz, use_log_depth=False) -> (dmaps [S,h,w], zrange [2])
                                                                                 the window's normalised depth and its range
    pack_weights(weight [128,191,3,3]) -> [24,9,8,128]                           the layout k_embed_conv stages (a permutation)
    embed_conv(fnet_maps [F,128,h,w], dmaps [S,h,w], zrange [2], frame0, conv, freqs, out=None) -> [F,128,h,w]
                                                                                 `embedConv` over the encoder's maps and the
                                                                                 Fourier embedding of (x, y, z), which is never
                                                                                 in memory; one launch
    sample_features(fmaps [S,128,h,w], frames [n], xy [n,>=2]) -> [n,128]        each query sampled from its own frame
    forward(self, rgbds, queries, iters=4, feat_init=None, is_train=False)       the window loop in our own words, the
                                                                                 reference's signature and return tuple;
                                                                                 `self.fnet` and `self.forward_iteration` are
                                                                                 called as they are
    forward_frames(self, frames, queries, iters=4)                               the single-window call on a `video.WindowFrames`:
                                                                                 the same loop on frames prepared and encoded once

Inference only (no autograd through the kernels), float32, GPU tensors only; no CPU fallback.  B = 1, 128 channels.

`install()` makes the reference's tracker use `forward` from here."""
import importlib
import weakref

import numpy as np
import torch

from .. import _lib
from ._conv import KCHUNK, _gpu, bias_of, cached, out_tensor, repack3x3  # noqa: F401  (KCHUNK stays a name of this module)

C = 128                      # BT_WINDOW_C (`latent_dim`)
EMB = 63                     # BT_WINDOW_EMB: Embedder_Fourier(3, N_freqs=10, include_input=True)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _workspace(device):
    """Zeroed: the ticket in its last word must be zero on entry; one per call, so that calls in flight share none."""
    return torch.zeros((_lib.lib().bt_window_workspace_bytes() + 3) // 4, dtype=torch.int32, device=device)


def depth_range(depth, use_log_depth=False):
    depth = _gpu("depth", depth, "depth_range")
    if depth.dim() != 3 or depth.numel() == 0:
        raise RuntimeError("depth_range: `depth` must be [T, H, W] and not empty")
    ops = _lib.torch_ops()
    if ops is not None:
        return ops.depth_range(depth, bool(use_log_depth))
    out, ws = torch.empty(2, dtype=torch.float32, device=depth.device), _workspace(depth.device)
    _lib.check(_lib.lib().bt_depth_range(depth.data_ptr(), *depth.shape, *depth.stride(), int(bool(use_log_depth)), ws.data_ptr(),
                                         out.data_ptr(), _stream(depth)), "bt_depth_range")
    return out


def window_depth(depth, S, stride, d_near, d_far, Dz, use_log_depth=False):
    """`depth` holds the window's frames (fewer than S: the last one is repeated).  d_near and d_far are Python floats; their
    difference is taken in double and rounded once, as the reference's `(d_far - d_near)` is."""
    depth = _gpu("depth", depth, "window_depth")
    S, stride = int(S), int(stride)
    if depth.dim() != 3 or depth.numel() == 0 or not 1 <= depth.shape[0] <= S:
        raise RuntimeError("window_depth: `depth` must be [frames, H, W] with 1 <= frames <= S and not empty")
    if stride < 1 or depth.shape[1] < stride or depth.shape[2] < stride:
        raise RuntimeError("window_depth: the stride must be positive and no larger than the image")
    d_range = float(d_far) - float(d_near)
    ops = _lib.torch_ops()
    if ops is not None:
        return ops.window_depth(depth, S, stride, float(d_near), d_range, float(Dz), bool(use_log_depth))
    h, w = depth.shape[1] // stride, depth.shape[2] // stride
    dmaps = torch.empty(S, h, w, dtype=torch.float32, device=depth.device)
    zrange, ws = torch.empty(2, dtype=torch.float32, device=depth.device), _workspace(depth.device)
    _lib.check(_lib.lib().bt_window_depth(depth.data_ptr(), depth.shape[0], S, depth.shape[1], depth.shape[2], *depth.stride(), stride,
                                          float(d_near), d_range, float(Dz), int(bool(use_log_depth)), ws.data_ptr(), dmaps.data_ptr(),
                                          zrange.data_ptr(), _stream(depth)), "bt_window_depth")
    return dmaps, zrange


def pack_weights(weight):
    """[128, 191, 3, 3] -> [24, 9, 8, 128]: packed[c // 8, 3 ky + kx, c % 8, o] = weight[o, c, ky, kx], zero for the padding
    channel 191.  A permutation of the weights (any device)."""
    if tuple(weight.shape) != (C, C + EMB, 3, 3):
        raise RuntimeError(f"embed_conv: the convolution must be 3 x 3 from {C + EMB} to {C} channels, not {tuple(weight.shape)}")
    w = weight.detach().float()
    return repack3x3(torch.cat([w, w.new_zeros(C, 1, 3, 3)], 1))


_packed = weakref.WeakKeyDictionary()        # conv -> (key, packed weight, bias)
_freqs = {}


def packed_conv(conv):
    """The module's repacked weight and its bias, redone when either tensor is replaced or written to."""
    w, b = conv.weight, conv.bias
    if b is None:
        raise RuntimeError("embed_conv: the convolution has no bias")
    if tuple(conv.padding) != (1, 1) or tuple(conv.stride) != (1, 1) or tuple(conv.dilation) != (1, 1) or conv.groups != 1 \
            or getattr(conv, "padding_mode", "zeros") != "zeros":
        raise RuntimeError("embed_conv: the convolution must have padding 1 (zeros), stride 1, no dilation and one group")
    return cached(_packed, conv, (w, b), lambda: (pack_weights(w), bias_of(conv)))


def freq_table(freqs, device):
    """The module's `freq_bands` as ten float32 on the device, taken as they are."""
    key = (tuple(float(f) for f in freqs), str(device))
    if len(key[0]) != 10:
        raise RuntimeError(f"embed_conv: the embedding must have 10 frequencies, not {len(key[0])}")
    if key not in _freqs:
        if len(_freqs) >= 8:                 # a model has one table: anything more is churn
            _freqs.clear()
        _freqs[key] = torch.tensor(key[0], dtype=torch.float32, device=device)
    return _freqs[key]


def embed_conv(fnet_maps, dmaps, zrange, frame0, conv, freqs, out=None):
    """`fnet_maps` [F, 128, h, w] (any strides) are frames frame0 .. frame0 + F of the window whose depth maps `dmaps` [S, h, w]
    and range `zrange` are; `out`, when given, is a contiguous [F, 128, h, w] (a slice of the window's buffer)."""
    fnet_maps, dmaps, zrange = (_gpu(n, t, "embed_conv") for n, t in (("fnet_maps", fnet_maps), ("dmaps", dmaps), ("zrange", zrange)))
    if fnet_maps.dim() != 4 or fnet_maps.shape[1] != C:
        raise RuntimeError(f"embed_conv: `fnet_maps` must be [F, {C}, h, w], not {tuple(fnet_maps.shape)}")
    F, __, h, w = fnet_maps.shape
    if h < 2 or w < 2:
        raise RuntimeError("embed_conv: maps of fewer than 2 rows or columns have no x or y range to normalise by")
    dmaps = dmaps.reshape(-1, h, w).contiguous()
    S, frame0 = dmaps.shape[0], int(frame0)
    if frame0 < 0 or frame0 + F > S or zrange.numel() != 2:
        raise RuntimeError("embed_conv: frames frame0 .. frame0 + F must lie in the window of `dmaps`, and `zrange` be its (min, max)")
    wp, bias = packed_conv(conv)
    if not wp.is_cuda or wp.device != fnet_maps.device:
        raise RuntimeError("embed_conv: the convolution must be on the GPU of the maps (there is no CPU fallback in batrack_amd)")
    ft = freq_table(freqs, fnet_maps.device)
    # as lenient as it was: an `out` on another GPU than the maps is not refused here
    out = out_tensor(out, (F, C, h, w), fnet_maps.device, "embed_conv", f"a contiguous float32 [F, {C}, h, w] on the GPU", same_device=False)
    zrange = zrange.contiguous()
    ops = _lib.torch_ops()
    if ops is not None:
        ops.embed_conv(fnet_maps, dmaps, zrange, wp, bias, ft, frame0, out)
    elif F:
        _lib.check(_lib.lib().bt_embed_conv(fnet_maps.data_ptr(), *fnet_maps.stride(), dmaps.data_ptr(), zrange.data_ptr(), wp.data_ptr(),
                                            bias.data_ptr(), ft.data_ptr(), S, frame0, F, h, w, C, out.data_ptr(), _stream(fnet_maps)),
                   "bt_embed_conv")
    return out


def sample_features(fmaps, frames, xy):
    """fmaps [S, 128, h, w]; frames [n] (any integer type); xy [n, >= 2] with unit last stride (a row view of the coordinate
    state is read in place) -> [n, 128]."""
    fmaps, xy = _gpu("fmaps", fmaps, "sample_features"), _gpu("xy", xy, "sample_features")
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise RuntimeError("sample_features: `frames` must be a tensor on the GPU (there is no CPU fallback in batrack_amd)")
    if fmaps.dim() != 4 or fmaps.shape[1] != C or fmaps.numel() == 0:
        raise RuntimeError(f"sample_features: `fmaps` must be [S, {C}, h, w], not {tuple(fmaps.shape)}")
    n = frames.numel()
    if xy.dim() != 2 or xy.shape[0] != n or xy.shape[1] < 2:
        raise RuntimeError("sample_features: `xy` must be [n, >= 2], a row per entry of `frames`")
    fmaps, frames = fmaps.contiguous(), frames.reshape(-1).to(torch.int32).contiguous()
    if xy.stride(1) != 1 or (n > 1 and xy.stride(0) < 2):
        xy = xy.contiguous()
    ops = _lib.torch_ops()
    if ops is not None:
        return ops.feat_sample(fmaps, frames, xy)
    out = torch.empty(n, C, dtype=torch.float32, device=fmaps.device)
    if n:
        _lib.check(_lib.lib().bt_feat_sample(fmaps.data_ptr(), *fmaps.shape, frames.data_ptr(), xy.data_ptr(), xy.stride(0) if n > 1 else 2,
                                             n, out.data_ptr(), _stream(fmaps)), "bt_feat_sample")
    return out


def _div_rn(a, b):
    """a / float32(b), correctly rounded, as the reference's CPU run divides a float32 tensor by a Python number.  (torch on
    the GPU multiplies by the reciprocal of a scalar divisor, which rounds twice.)  The quotient of two float32 values taken
    in double and rounded to float32 is the correctly rounded float32 quotient."""
    return (a.double() / torch.full((), float(np.float32(b)), dtype=torch.float64, device=a.device)).float()


def _checked(self, what):
    """(S, stride, use_log_depth) of the tracker `self`, or a RuntimeError naming what `what` cannot run on."""
    S, stride = int(self.S), int(self.stride)
    if S % 2 or stride < 1 or stride & (stride - 1):
        raise RuntimeError(f"{what}: the window length must be even and the stride a power of two")
    if int(self.latent_dim) != C:
        raise RuntimeError(f"{what}: latent_dim must be {C}")
    return S, stride, bool(getattr(self, "use_log_depth", False))


def forward(self, rgbds, queries, iters=4, feat_init=None, is_train=False):
    if is_train:
        raise RuntimeError("tracker.forward: inference only (is_train=True is not supported)")
    _gpu("rgbds", rgbds, "tracker.forward")
    _gpu("queries", queries, "tracker.forward")
    B, T, C_img, H, W = rgbds.shape
    if queries.shape[0] != 1:                                               # (the queries' batch, as before)
        raise RuntimeError("tracker.forward: B must be 1")
    S, stride, use_log = _checked(self, "tracker.forward")

    # the caller's rgbds, in place; the division goes through double, in chunks of frames that keep that temporary to 64 MB
    step = max(1, (1 << 23) // max(1, 3 * H * W))
    for t in range(0, T, step):
        rgbds[:, t: t + step, :3] = 2 * _div_rn(rgbds[:, t: t + step, :3], 255.0) - 1.0
    d_near, d_far = depth_range(rgbds[0, :, 3], use_log).tolist()           # the other read-back

    def fnet_of(ind, lo, hi):
        rgbs_ = rgbds[0, ind: ind + S, :3]
        if rgbs_.shape[0] < S:                                              # a short last window repeats its last frame
            rgbs_ = torch.cat([rgbs_, rgbs_[-1:].repeat(S - rgbs_.shape[0], 1, 1, 1)], dim=0)
        return self.fnet(rgbs_[lo:hi])

    return _windows(self, queries, iters, feat_init, T, H, W, d_near, d_far, lambda ind, S_local: rgbds[0, ind: ind + S_local, 3], fnet_of,
                    "tracker.forward", (S, stride, use_log))


def forward_frames(self, frames, queries, iters=4):
    """The tracker's single-window call on a `video.WindowFrames`: `forward`'s tuple for the window's frames, with what each
    frame's preparation and encoding cost paid once per frame and not once per call.  A window shorter than S repeats its last
    frame (the maps and the depth are copied, not recomputed).  One host read: the depth range.

    Bit-equal to `forward(self, rgbds, queries, iters)` on the same S frames — prepared by `video.prepare_frames(normalise=False)`
    and padded as `get_window_trajs` pads them — whenever `frames.fnet` is `self.fnet` and a frame's maps do not depend on the
    frames encoded with it."""
    _gpu("queries", queries, "tracker.forward_frames")
    if queries.shape[0] != 1:
        raise RuntimeError("tracker.forward_frames: B must be 1")
    S, stride, use_log = _checked(self, "tracker.forward_frames")
    if int(frames.S) != S or bool(frames.use_log_depth) != use_log:
        raise RuntimeError("tracker.forward_frames: the frames' window length and use_log_depth must be the tracker's")
    rgbd, maps, drange = frames.window()
    n = rgbd.shape[0]
    if maps.shape[1] != C or tuple(maps.shape[2:]) != (rgbd.shape[2] // stride, rgbd.shape[3] // stride):
        raise RuntimeError(f"tracker.forward_frames: the frames' maps must be [n, {C}, H / stride, W / stride], not {tuple(maps.shape)}")
    if n < S:
        maps = torch.cat([maps, maps[-1:].expand(S - n, -1, -1, -1)], dim=0)
    d_near, d_far = drange.tolist()
    return _windows(self, queries, iters, None, S, rgbd.shape[2], rgbd.shape[3], d_near, d_far, lambda ind, S_local: rgbd[:, 3],
                    lambda ind, lo, hi: maps[lo:hi], "tracker.forward_frames", (S, stride, use_log))


def _windows(self, queries, iters, feat_init, T, H, W, d_near, d_far, depth_of, fnet_of, what, checked):
    """The window loop `forward` and `forward_frames` share, from the depth range on.  depth_of(ind, S_local) is the depth
    [<= S_local, H, W] of the window that starts at frame `ind` (fewer frames: the last is repeated); fnet_of(ind, lo, hi) the
    encoder's maps of that window's frames lo .. hi, its padding frames included."""
    B, N, __ = queries.shape
    device = queries.device
    S, stride, use_log = checked                                            # of `_checked(self, what)`, by the caller
    half = S // 2

    first_positive_inds = queries[:, :, 0].long()
    __, sort_inds = torch.sort(first_positive_inds[0], dim=0, descending=False, stable=True)      # ties as the reference's CPU sort leaves them
    inv_sort_inds = torch.argsort(sort_inds, dim=0)
    first_positive_sorted_inds = first_positive_inds[0][sort_inds]
    first_sorted_host = first_positive_sorted_inds.cpu().numpy()            # one read-back: the windows' track counts

    if not (np.isfinite(d_near) and np.isfinite(d_far)):
        raise RuntimeError(f"{what}: the video has no depth above 0.01, or a NaN depth (use_log_depth)")
    self.d_near, self.d_far = d_near, d_far
    self.Dz = Dz = W // stride
    d_range = d_far - d_near
    depth_norm = lambda d: _div_rn(self.depth_process(d) - d_near, d_range)

    traj_e = torch.zeros((B, T, N, 2), device=device)
    depth_e = torch.zeros((B, T, N, 1), device=device)
    traj_static_e = torch.zeros((B, T, N, 3), device=device)
    vis_e = torch.zeros((B, T, N), device=device)
    dynamic_e = torch.zeros((B, T, N), device=device)

    ind_array = torch.arange(T, device=device)[None, :, None].repeat(B, 1, N)
    track_mask = (ind_array >= first_positive_inds[:, None, :]).unsqueeze(-1)
    vis_init = torch.ones((B, S, N, 1), device=device).float() * 10
    coords_init = queries[:, :, 1:].reshape(B, 1, N, 3).repeat(1, S, 1, 1)
    coords_init[..., :2] /= float(stride)
    coords_init[..., 2] = depth_norm(coords_init[..., 2])
    coords_init[..., 2] *= Dz

    ind = 0
    track_mask_ = track_mask[:, :, sort_inds].clone()
    coords_init_ = coords_init[:, :, sort_inds].clone()
    coords_dyn_init_ = torch.zeros_like(coords_init_)
    vis_init_ = vis_init[:, :, sort_inds].clone()

    prev_wind_idx = 0
    fmaps_ = None
    h, w = H // stride, W // stride
    while ind < T - half:
        S_local = min(S, T - ind)
        dmaps_, zrange = window_depth(depth_of(ind, S_local), S, stride, d_near, d_far, Dz, use_log)

        if self.Embed3D:
            freqs = self.embed3d.freq_bands
            if fmaps_ is None:
                fmaps_ = embed_conv(fnet_of(ind, 0, S), dmaps_, zrange, 0, self.embedConv, freqs)
            else:                                                           # a slide: the old second half, and the new half convolved
                window = torch.empty_like(fmaps_)
                window[:half] = fmaps_[half:]
                embed_conv(fnet_of(ind, half, S), dmaps_, zrange, half, self.embedConv, freqs, out=window[half:])
                fmaps_ = window
        elif fmaps_ is None:
            fmaps_ = fnet_of(ind, 0, S)
        else:
            fmaps_ = torch.cat([fmaps_[half:], fnet_of(ind, half, S)], dim=0)

        fmaps = fmaps_[:, :C].reshape(B, S, C, h, w)
        dmaps = dmaps_.reshape(B, S, 1, h, w)

        wind_idx = int((first_sorted_host < ind + S).sum())
        if wind_idx == 0:                                                   # no query yet
            ind = ind + half
            continue

        if wind_idx - prev_wind_idx > 0:
            feat_init_ = sample_features(fmaps[0], first_positive_sorted_inds[prev_wind_idx:wind_idx] - ind,
                                         coords_init_[0, 0, prev_wind_idx:wind_idx])
            feat_init_ = feat_init_[None, None].repeat(1, S, 1, 1)
            feat_init = feat_init_ if feat_init is None else torch.cat([feat_init, feat_init_], dim=2)

        if prev_wind_idx > 0:
            new_coords_2d = coords[-1][:, half:].clone()
            new_coords_2d /= float(stride)
            new_coords_depth = depth_norm(coords_depth[-1][:, half:].clone()) * Dz
            new_coords = torch.cat([new_coords_2d, new_coords_depth], dim=-1)
            coords_init_[:, :half, :prev_wind_idx] = new_coords
            coords_init_[:, half:, :prev_wind_idx] = new_coords[:, -1].repeat(1, half, 1, 1)

            # the dynamic flow, as the reference carries it (md_tracker.py:597-608)
            new_coords_dyn_2d = new_coords_2d - coords_static_3d[-1][:, half:, :, :2].clone()
            new_coords_dyn_2d /= float(stride)
            new_coords_dyn_depth = new_coords_depth - coords_static_3d[-1][:, half:, :, 2:].clone()
            new_coords_dyn_depth = depth_norm(new_coords_dyn_depth) * Dz
            new_coords_dyn = torch.cat([new_coords_dyn_2d, new_coords_dyn_depth], dim=-1)
            coords_dyn_init_[:, :half, :prev_wind_idx] = new_coords_dyn
            coords_dyn_init_[:, half:, :prev_wind_idx] = new_coords_dyn[:, -1].repeat(1, half, 1, 1)

            new_vis = vis[:, half:].unsqueeze(-1)
            vis_init_[:, :half, :prev_wind_idx] = new_vis
            vis_init_[:, half:, :prev_wind_idx] = new_vis[:, -1].repeat(1, half, 1, 1)

        coords, coords_depth, coords_static_3d, vis, dynamic, __ = self.forward_iteration(
            fmaps=fmaps,
            dmaps=dmaps,
            coords_init=coords_init_[:, :, :wind_idx],
            coords_dyn_init=coords_dyn_init_[:, :, :wind_idx],
            feat_init=feat_init[:, :, :wind_idx],
            vis_init=vis_init_[:, :, :wind_idx],
            track_mask=track_mask_[:, ind: ind + S, :wind_idx],
            iters=iters,
        )

        traj_e[:, ind: ind + S, :wind_idx] = coords[-1][:, :S_local]
        depth_e[:, ind: ind + S, :wind_idx] = coords_depth[-1][:, :S_local]
        traj_static_e[:, ind: ind + S, :wind_idx] = coords_static_3d[-1][:, :S_local]
        vis_e[:, ind: ind + S, :wind_idx] = vis[:, :S_local]
        dynamic_e[:, ind: ind + S, :wind_idx] = dynamic[:, None].expand(-1, S_local, -1)

        track_mask_[:, : ind + S, :wind_idx] = 0.0
        ind = ind + half
        prev_wind_idx = wind_idx

    traj_e = traj_e[:, :, inv_sort_inds]
    depth_e = depth_e[:, :, inv_sort_inds]
    traj_static_e = traj_static_e[:, :, inv_sort_inds]
    vis_e = torch.sigmoid(vis_e[:, :, inv_sort_inds])
    dynamic_e = torch.sigmoid(dynamic_e[:, :, inv_sort_inds])
    return traj_e, feat_init, depth_e, traj_static_e, vis_e, dynamic_e, None


def install(module=None):
    """Set `MDTracker.forward` in the reference's tracker module (`main.frontend.md_tracker`, or the module given) to
    `forward` above; returns what was bound before.  Opt-in: nothing in batrack_amd calls it."""
    if module is None:
        module = importlib.import_module("main.frontend.md_tracker")
    previous = getattr(module.MDTracker, "forward", None)
    module.MDTracker.forward = forward
    return previous
