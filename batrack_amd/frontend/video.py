"""What feeds the tracker (the reference's main/batrack.py: `preprocess`, :385-392, `get_window_trajs`, :667-700, and
`_compute_sparse_tracks`, :529-587): the frames of the local window resized to the tracker's size, their colours mapped to
[-1, 1] and their depth range taken, HIP underneath (batrack_amd/csrc/video_prep.hip through include/batrack_video.h, which
holds the specification), and a per-frame cache of that and of the encoder's maps.

    prepare_frames(image [F,3,H,W], depth [F,H,W], size=(384, 512), normalise=True, use_log_depth=False, out=None)
        -> (rgbd [F,4,oh,ow], drange [F,2])            resize with the exact source coordinate, colour mapping, each frame's
                                                       masked depth range; one launch; uint8 or float32 images, any strides
    compute_sparse_tracks(self, rgbds, queries)        `BATRACK._compute_sparse_tracks` in our own words, the reference's
                                                       signature and return tuple; `self.network` is called as it is
    WindowFrames(S, fnet, size=(384, 512), use_log_depth=False)
                                                       the local window with each frame prepared and encoded ONCE: push(image,
                                                       depth), window() -> (rgbd, fmaps, drange), len(), clear()
    tracker.forward_frames(self, frames, queries, iters=4)   the tracker's single-window call on a WindowFrames (tracker.py)

Inference only, float32 out, GPU tensors only; no CPU fallback.

`install()` makes the reference's BATRACK use `compute_sparse_tracks` from here."""
import importlib

import torch

from .. import _lib
from ._conv import _gpu, out_tensor

SIZE = (384, 512)            # the reference's interp_shape


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


_workspaces = {}             # (device, stream, ticket words) -> int32 words, zero when made; the kernel leaves the tickets zero


def _workspace(device, F, nbytes):
    """The workspace of the device's current stream for calls of F frames, made (zeroed, once) or grown on demand: calls on one
    stream run one after the other, so they may share it, and no call pays for an allocation or a memset.  One per number of
    ticket words, 4 ceil(F / 4): the blocks' pairs begin where the tickets end, so a call with more frames would find another
    call's pairs where it expects zero tickets."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, (F + 3) // 4 * 4)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = _workspaces[key] = torch.zeros(max(4096, (nbytes + 3) // 4), dtype=torch.int32, device=device)
    return ws


def _check_frames(image, depth, what):
    depth = _gpu("depth", depth, what)
    if not isinstance(image, torch.Tensor) or not image.is_cuda:
        raise RuntimeError(f"{what}: `image` must be a tensor on the GPU (there is no CPU fallback in batrack_amd)")
    if image.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"{what}: `image` must be uint8 or float32, not {image.dtype}")
    if image.dim() != 4 or image.shape[1] != 3 or depth.dim() != 3 or tuple(depth.shape) != (image.shape[0], image.shape[2], image.shape[3]):
        raise RuntimeError(f"{what}: `image` must be [F, 3, H, W] and `depth` [F, H, W], not {tuple(image.shape)} and {tuple(depth.shape)}")
    if image.shape[2] < 1 or image.shape[3] < 1:
        raise RuntimeError(f"{what}: the frames must not be empty")
    if image.device != depth.device:
        raise RuntimeError(f"{what}: `image` and `depth` must be on one GPU")
    return image.detach(), depth


def prepare_frames(image, depth, size=SIZE, normalise=True, use_log_depth=False, out=None):
    """image [F, 3, H, W] uint8 or float32 (any strides: the permuted view of an HWC array is read in place), depth [F, H, W]
    float32 (any strides) -> rgbd [F, 4, oh, ow] (`out`, when given: a contiguous float32 tensor of that shape, e.g. a slice of
    a window's buffer) and drange [F, 2], each frame's (min, max) by `tracker.depth_range`'s rules.  One launch: the workspace is
    kept per device, stream and ticket count (`_workspace`), zeroed when it is made and left with zero tickets by every call."""
    image, depth = _check_frames(image, depth, "prepare_frames")
    oh, ow = (int(v) for v in size)
    if oh < 1 or ow < 1:
        raise RuntimeError("prepare_frames: the output size must be at least 1 x 1")
    F, __, H, W = image.shape
    rgbd = out_tensor(out, (F, 4, oh, ow), depth.device, "prepare_frames", "a contiguous float32 [F, 4, oh, ow] on the GPU of the frames")
    drange = torch.empty(F, 2, dtype=torch.float32, device=depth.device)
    if F == 0:
        return rgbd, drange
    L = _lib.lib()
    nbytes = L.bt_frame_prep_workspace_bytes(F, oh, ow)
    if nbytes == 0:
        raise RuntimeError("prepare_frames: " + _lib.ERRORS[_lib.BT_EUNSUPPORTED])
    ws = _workspace(depth.device, F, nbytes)
    ops = _lib.torch_ops()
    if ops is not None:
        ops.frame_prep(image, depth, bool(normalise), bool(use_log_depth), ws, rgbd, drange)
        return rgbd, drange
    _lib.check(L.bt_frame_prep(image.data_ptr(), int(image.dtype == torch.uint8), *image.stride(), depth.data_ptr(), *depth.stride(),
                               F, H, W, oh, ow, int(bool(normalise)), int(bool(use_log_depth)), ws.data_ptr(), rgbd.data_ptr(),
                               drange.data_ptr(), _stream(depth)), "bt_frame_prep")
    return rgbd, drange


def _flag(node, name):
    """`name in node and node.name`, for a config node that is a mapping or a plain namespace."""
    return bool(node.get(name, False)) if hasattr(node, "get") else bool(getattr(node, name, False))


def compute_sparse_tracks(self, rgbds, queries):
    """rgbds [1, T, 4, H, W] (colours 0 .. 255 and depth, as `get_window_trajs` stacks them), queries [1, N, 4] (frame, x, y,
    depth) -> (tracks [1, T, N, 2] in image pixels, depths, visibilities, stats).  The network normalises the colours of the
    resized frames it is given in place, ours and the reference's alike, so they are prepared with normalise=False."""
    _gpu("rgbds", rgbds, "compute_sparse_tracks")
    _gpu("queries", queries, "compute_sparse_tracks")
    if rgbds.dim() != 5 or rgbds.shape[0] != 1 or rgbds.shape[2] != 4:
        raise RuntimeError(f"compute_sparse_tracks: `rgbds` must be [1, T, 4, H, W], not {tuple(rgbds.shape)}")
    if queries.dim() != 3 or queries.shape[2] != 4:
        raise RuntimeError(f"compute_sparse_tracks: `queries` must be [B, N, 4], not {tuple(queries.shape)}")
    cfg = self.cfg
    if cfg.model.mode not in ("md_tracker",):
        raise RuntimeError(f"compute_sparse_tracks: model.mode must be \"md_tracker\", not {cfg.model.mode!r}")
    if cfg.slam.backward_tracking and self.S_slam > cfg.model.S:
        raise RuntimeError("compute_sparse_tracks: backward tracking over a window longer than the model's (S_slam > model.S) is not supported")
    __, T, __, H, W = rgbds.shape
    oh, ow = (int(v) for v in self.interp_shape)
    rgbd, __ = prepare_frames(rgbds[0, :, :3], rgbds[0, :, 3], (oh, ow), normalise=False)

    queries = queries.clone()
    queries[:, :, 1] *= ow / W
    queries[:, :, 2] *= oh / H

    tracks, __, depths, traj_static_3d_e, visibilities, dynamic_e, __ = self.network(rgbds=rgbd[None], queries=queries, iters=cfg.model.I)
    if _flag(cfg.model, "use_static_mask"):
        dyn_mask = dynamic_e > (1 - cfg.slam.STATIC_THRESHOLD)
        tracks[dyn_mask] = traj_static_3d_e[..., :2][dyn_mask]
        depths[dyn_mask] = traj_static_3d_e[..., 2:][dyn_mask]
    if _flag(cfg.model, "use_static"):
        tracks, depths = traj_static_3d_e[..., :2], traj_static_3d_e[..., 2:]
    stats = {"dynamic_e": dynamic_e}

    n = tracks.size(2)
    columns = torch.arange(n, device=tracks.device)
    for i in range(queries.shape[0]):                           # the predictions at the query frames are the queries
        frames_i = queries[i, :n, 0].to(torch.int64)
        tracks[i, frames_i, columns] = queries[i, :n, 1:3]
        visibilities[i, frames_i, columns] = 1.0
    tracks[:, :, :, 0] *= W / float(ow)
    tracks[:, :, :, 1] *= H / float(oh)
    return tracks, depths, visibilities, stats


class WindowFrames:
    """The local window of `S` frames (`BATRACK.preprocess`), each frame prepared and encoded once.

    push(image [3, H, W] uint8 or float32, depth [H, W]) appends a frame and drops the oldest beyond S; nothing is launched.
    window() -> (rgbd [n, 4, oh, ow] with normalised colours, fmaps [n, 128, h, w], drange [2]) in window order: the frames
    pushed since the last window() go through ONE `prepare_frames(normalise=True)` and ONE `fnet` call into their slots.
    drange is the NaN-propagating (min, max) over the frames' pairs, on the device.

    Window order costs no copy per call: the frames lie in a buffer of 2 S slots in the order they came, and a window is a
    view of n consecutive slots.  When the buffer's end is reached the frames that stay are copied to its front: one copy of
    at most S - 1 frames (rgbd and maps) every S or more pushed frames, and twice the window's memory (at S = 12 and 384 x 512:
    2 x 113 MB).  The views a window() returned are valid until the next window()."""

    def __init__(self, S, fnet, size=SIZE, use_log_depth=False):
        self.S, self.fnet, self.size, self.use_log_depth = int(S), fnet, tuple(int(v) for v in size), bool(use_log_depth)
        if self.S < 1:
            raise RuntimeError("WindowFrames: S must be at least 1")
        self.clear()

    def clear(self):
        self._pending, self._count, self._end = [], 0, 0
        self._rgbd = self._fmaps = self._drange = None

    def __len__(self):
        return min(self.S, self._count + len(self._pending))

    def push(self, image, depth):
        if not isinstance(image, torch.Tensor) or image.dim() != 3 or not isinstance(depth, torch.Tensor) or depth.dim() != 2:
            raise RuntimeError("WindowFrames.push: `image` must be a [3, H, W] tensor and `depth` a [H, W] tensor")
        image, depth = _check_frames(image[None], depth[None], "WindowFrames.push")
        self._pending.append((image[0], depth[0]))
        del self._pending[:-self.S]

    def window(self):
        k = len(self._pending)
        if self._count + k == 0:
            raise RuntimeError("WindowFrames.window: no frame has been pushed")
        if k:
            image = torch.stack([p[0] for p in self._pending])
            depth = torch.stack([p[1] for p in self._pending])
            self._pending = []
            oh, ow = self.size
            if self._rgbd is None:
                self._rgbd = torch.empty(2 * self.S, 4, oh, ow, dtype=torch.float32, device=depth.device)
                self._drange = torch.empty(2 * self.S, 2, dtype=torch.float32, device=depth.device)
            keep = min(self._count, self.S - k)
            if self._end + k > 2 * self.S:                      # the slide to the front: [end - keep, end) and [0, keep) do not overlap
                for buf in (self._rgbd, self._fmaps, self._drange):
                    buf[:keep] = buf[self._end - keep: self._end]
                self._end = keep
            lo, hi = self._end, self._end + k
            __, dr = prepare_frames(image, depth, self.size, True, self.use_log_depth, out=self._rgbd[lo:hi])
            self._drange[lo:hi] = dr
            maps = self.fnet(self._rgbd[lo:hi, :3])
            if self._fmaps is None:
                if maps.dim() != 4 or maps.shape[0] != k:
                    raise RuntimeError(f"WindowFrames.window: `fnet` must return [F, C, h, w] for F frames, not {tuple(maps.shape)}")
                self._fmaps = torch.empty(2 * self.S, *maps.shape[1:], dtype=torch.float32, device=depth.device)
            self._fmaps[lo:hi] = maps
            self._end, self._count = hi, keep + k
        w = slice(self._end - self._count, self._end)
        dr = self._drange[w]
        return self._rgbd[w], self._fmaps[w], torch.stack([dr[:, 0].min(), dr[:, 1].max()])


def install(module=None):
    """Set `BATRACK._compute_sparse_tracks` in the reference's module (`main.batrack`, or the module given) to
    `compute_sparse_tracks` above; returns what was bound before.  Opt-in: nothing in batrack_amd calls it."""
    if module is None:
        module = importlib.import_module("main.batrack")
    previous = getattr(module.BATRACK, "_compute_sparse_tracks", None)
    module.BATRACK._compute_sparse_tracks = compute_sparse_tracks
    return previous
