"""From the tracker's window output to what the bundle adjustment consumes, on the device: the reference's
`predict_target` -> `get_window_trajs` -> `_compute_sparse_tracks` (tail) -> `update_local` (main/batrack.py:760-818,
667-757, 575-587, 632-663) as one call of bt_observe_window (batrack_amd/csrc/observe.hip; include/batrack_observe.h
holds the specification): at most three launches, no host round trip — the motion-decoupling threshold (a quantile the
reference fetches with `.item()`) stays in device memory.

    targets_3d, weights, weights_pose, query_disp = window_observations(
        traj [1,S,Nq,2], depth [1,S,Nq,1], vis [1,S,Nq], dyn [1,S,Nq], queries [1,Nq,3], dmaps [S',H,W] or None,
        ii, jj, kk,  patches_valid=..., patches_local=..., ..., n=..., window=S', kf_stride=..., wd=..., ht=..., cfg=...)

`traj`, `depth`, `vis`, `dyn` are what the tracker network returns (before the tail of `_compute_sparse_tracks`, which
the kernel applies on load); `queries` is `get_queries()`; `ii, jj, kk` are the new edges (`ii_new, jj_new, kk_new`).
The buffers are updated in place.  Returns targets_3d [1,E,3], weights [1,E,2], weights_pose [1,E,2] (to be appended to
the caller's) and query_disp [Nq] (`patches_monodisp_` of the window's keyframes; None without `dmaps`).
GPU tensors only; no CPU fallback.  Not restated: the CONF_THRESHOLD / var_e branch, use_static_mask / use_static,
backward tracking."""
import ctypes
import dataclasses
from typing import Optional

import torch

from .. import _lib


@dataclasses.dataclass
class ObserveConfig:
    """The keys of the reference's `slam:` block this step reads (names kept; configs/sintel.yaml values)."""
    VIS_THRESHOLD: Optional[float] = 0.9          # None: the key is absent, every entry counts as visible
    STATIC_THRESHOLD: float = 0.1
    STATIC_QUANTILE: float = 0.0
    MIN_TRACK_LEN: int = 3


_workspace = {}


def _ws(device):
    """The call's scratch (the threshold): one small tensor per device, reused — calls on one stream are ordered."""
    w = _workspace.get(device)
    if w is None:
        w = _workspace[device] = torch.empty(max(_lib.lib().bt_observe_workspace_bytes() // 4, 1), dtype=torch.float32, device=device)
    return w


def _gpu(name, t, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"window_observations: `{name}` must be a tensor on the GPU (there is no CPU fallback in batrack_amd)")
    if t.dtype != dtype:
        raise RuntimeError(f"window_observations: `{name}` must be {dtype}")
    return t


def _inout(name, t, numel):
    if t is None:
        return None
    _gpu(name, t)
    if not t.is_contiguous() or t.numel() != numel:
        raise RuntimeError(f"window_observations: `{name}` must be contiguous with {numel} elements: it is updated in place")
    return t


def window_observations(traj, depth, vis, dyn, queries, dmaps, ii, jj, kk, *, patches_valid, patches_local, local_monodisp=None,
                        local_vis=None, local_static=None, local_weights=None, n, window, kf_stride, wd, ht, cfg=None,
                        is_initialized=False, interp_shape=(384, 512), image_size=None, padding=20):
    """See the module's text.  window: S' = len(local_window).  interp_shape: the tracker's (height, width), None = the
    tensors are already in full-image pixels with the queries written in (no tail).  image_size: (H, W) of the frames;
    taken from `dmaps` when they are given."""
    cfg = cfg or ObserveConfig()
    traj = _gpu("traj", traj)
    if traj.dim() != 4 or traj.shape[0] != 1 or traj.shape[3] != 2:
        raise RuntimeError("window_observations: `traj` must be [1, S, Nq, 2] (batch 1, as the reference asserts)")
    S, Nq = traj.shape[1], traj.shape[2]
    traj = traj.reshape(S, Nq, 2).contiguous()
    depth, vis, dyn = (_gpu(k, t).reshape(S, Nq).contiguous() for k, t in (("depth", depth), ("vis", vis), ("dyn", dyn)))
    queries = _gpu("queries", queries).reshape(Nq, 3).contiguous()
    Sp = int(window)
    if dmaps is not None:
        dmaps = _gpu("dmaps", dmaps)
        H, W = dmaps.shape[-2:]
        dmaps = dmaps.reshape(Sp, H, W).contiguous()
    elif image_size is not None:
        H, W = image_size
    elif interp_shape is None:
        H = W = 1                                   # unused without the tail and without maps
    else:
        raise RuntimeError("window_observations: the tail's rescale needs `image_size` = (H, W) when no `dmaps` are given")
    ii, jj, kk = (_gpu(k, t, torch.int64).reshape(-1).contiguous() for k, t in (("ii", ii), ("jj", jj), ("kk", kk)))
    _gpu("patches_valid", patches_valid)
    if patches_valid.dim() != 2 or not patches_valid.is_contiguous():
        raise RuntimeError("window_observations: `patches_valid` must be contiguous [N, M]: it is updated in place")
    N, M = patches_valid.shape
    _gpu("patches_local", patches_local)
    if not patches_local.is_contiguous() or patches_local.shape[-1] != 3 or patches_local.numel() % (3 * N * M):
        raise RuntimeError("window_observations: `patches_local` must be contiguous [..., S_local, 3] over the N*M tracks")
    S_local = patches_local.shape[-2]
    pl = patches_local.view(N * M, S_local, 3)
    opt = [_inout(k, t, N * M * S_local) for k, t in (("local_monodisp", local_monodisp), ("local_vis", local_vis),
                                                       ("local_static", local_static), ("local_weights", local_weights))]
    iw, ih = (int(interp_shape[1]), int(interp_shape[0])) if interp_shape is not None else (0, 0)
    vt = None if cfg.VIS_THRESHOLD is None else float(cfg.VIS_THRESHOLD)
    ws = _ws(traj.device)
    ops = _lib.torch_ops()
    if ops is not None:
        t3, w, wp, qd = ops.observe_window(traj, depth, vis, dyn, queries, dmaps, ii, jj, kk, patches_valid, pl, *opt, ws, int(n), Sp,
                                           int(kf_stride), int(H), int(W), float(wd), float(ht), int(padding), vt,
                                           float(cfg.STATIC_QUANTILE), float(cfg.STATIC_THRESHOLD), int(cfg.MIN_TRACK_LEN),
                                           bool(is_initialized), iw, ih)
    else:
        E = Nq * Sp
        f32 = dict(dtype=torch.float32, device=traj.device)
        t3, w, wp = torch.empty(E, 3, **f32), torch.empty(E, 2, **f32), torch.empty(E, 2, **f32)
        qd = torch.empty(Nq if dmaps is not None else 0, **f32)
        if ii.numel() != E or jj.numel() != E or kk.numel() != E:
            raise RuntimeError("window_observations: ii, jj, kk must hold Nq * window edges")
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        a = _lib.ObserveArgs(S=S, Sp=Sp, Nq=Nq, E=E, n=int(n), M=M, N=N, kf_stride=int(kf_stride), S_local=S_local, H=int(H), W=int(W),
                             interp_w=iw, interp_h=ih, padding=int(padding), min_track_len=int(cfg.MIN_TRACK_LEN),
                             has_vis_threshold=int(vt is not None), is_initialized=int(bool(is_initialized)), wd=float(wd), ht=float(ht),
                             vis_threshold=vt or 0.0, static_quantile=float(cfg.STATIC_QUANTILE), static_threshold=float(cfg.STATIC_THRESHOLD),
                             traj=traj.data_ptr(), depth=depth.data_ptr(), vis=vis.data_ptr(), dyn=dyn.data_ptr(), queries=queries.data_ptr(),
                             dmaps=ptr(dmaps), ii=ii.data_ptr(), jj=jj.data_ptr(), kk=kk.data_ptr(), patches_valid=patches_valid.data_ptr(),
                             patches_local=pl.data_ptr(), local_monodisp=ptr(opt[0]), local_vis=ptr(opt[1]), local_static=ptr(opt[2]),
                             local_weights=ptr(opt[3]), targets_3d=t3.data_ptr(), weights=w.data_ptr(), weights_pose=wp.data_ptr(),
                             query_disp=ptr(qd))
        st = torch.cuda.current_stream(traj.device).cuda_stream
        _lib.check(_lib.lib().bt_observe_window(ctypes.byref(a), ws.data_ptr(), st), "bt_observe_window")
    return t3[None], w[None], wp[None], (qd if dmaps is not None else None)
