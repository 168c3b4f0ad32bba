"""The last step of a frame on the device: the reference's `BATRACK.keyframe()` and `keyframe_simple()`
(main/batrack.py:1026-1073, 1020-1024) with the `motionmag` (:1011-1018) and `remove_factors` (:206-212) they are built
from, as one call: bt_keyframe_decide -> bt_edges_prune -> bt_rows_shift (batrack_amd/csrc/keyframe.hip;
include/batrack_keyframe.h holds the specification), at most six launches enqueued back to back, then the one host read
of the call — the 32-byte status, copied to a pinned buffer, and a stream synchronise.

    res = prune_keyframe(poses [N,7], patches [N*M,3,p,p], intrinsics [N,4], ii, jj, kk, targets_3d [1,E,3],
                         weights [1,E,2], weights_pose [1,E,2], n=..., M=..., kf_stride=..., cfg=KeyframeConfig(),
                         frame_buffers=(tstamps_, poses_, ...), candidate=True)

candidate=True is `keyframe()`: k = n - KEYFRAME_INDEX; when k % kf_stride != 0 the reference returns before it does
anything (:1030-1031), so the inputs come back untouched, nothing is launched and the removal window is NOT applied.
candidate=False is `keyframe_simple()`: only the removal window.  `frame_buffers`: the per-frame tensors (contiguous,
leading dimension N) whose rows k+1 .. n-1 move down by one, in place, when the frame is removed.  `res.dP` is
SE3(poses[k]) * SE3(poses[k-1])^-1, enqueued before the shift with the SE3 kernels ([7] tensor; None when nothing was
removed).  The returned edge tensors are `[:E_out]` views of fresh outputs.  GPU tensors only; no CPU fallback."""
import collections
import dataclasses

import torch

from .. import _lib


@dataclasses.dataclass
class KeyframeConfig:
    """The keys of the reference's `slam:` block this step reads (names kept; configs/davis_demo.yaml values)."""
    KEYFRAME_INDEX: int = 4
    KEYFRAME_THRESH: float = 10.0
    REMOVAL_WINDOW: int = 20
    beta: float = 0.5                 # motionmag's flow_mag(..., beta=0.5), batrack.py:1017


KeyframeResult = collections.namedtuple("KeyframeResult", "removed k ii jj kk targets_3d weights weights_pose mag_prev mag_next dP")

_workspace = {}
_pinned = {}


def _ws(device, E):
    """The call's scratch, status word first: one tensor per device, grown when the edge list does; calls on one stream are ordered."""
    need = _lib.lib().bt_keyframe_workspace_bytes(E)
    w = _workspace.get(device)
    if w is None or w.numel() * 8 < need:
        w = _workspace[device] = torch.empty((2 * need + 7) // 8, dtype=torch.int64, device=device)
    return w


def _host_status(device):
    h = _pinned.get(device)
    if h is None:
        h = _pinned[device] = torch.empty(4, dtype=torch.int64).pin_memory()
    return h


def _gpu(name, t, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"prune_keyframe: `{name}` must be a tensor on the GPU (there is no CPU fallback in batrack_amd)")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"prune_keyframe: `{name}` must be {dtype}")
    return t


def prune_keyframe(poses, patches, intrinsics, ii, jj, kk, targets_3d, weights, weights_pose, *, n, M, kf_stride, cfg=None,
                   frame_buffers=(), candidate=True):
    """See the module's text."""
    cfg = cfg or KeyframeConfig()
    n, M = int(n), int(M)
    nothing = lambda k: KeyframeResult(False, k, ii, jj, kk, targets_3d, weights, weights_pose, float("nan"), float("nan"), None)
    k = -1
    if candidate:
        k = n - int(cfg.KEYFRAME_INDEX)
        if k % int(kf_stride) != 0:
            for name, t in (("ii", ii), ("poses", poses)):
                _gpu(name, t, None)
            return nothing(k)                                   # batrack.py:1030-1031
        if k < 0:
            k = -1                                              # no frame there: no edge can name it
    P = _gpu("poses", poses).reshape(-1, 7)
    pat = _gpu("patches", patches)
    pat = pat.reshape(-1, *pat.shape[-3:])
    K = _gpu("intrinsics", intrinsics).reshape(-1, 4)
    if pat.shape[1] != 3 or pat.shape[2] != pat.shape[3]:
        raise RuntimeError("prune_keyframe: `patches` must be [N*M, 3, p, p]")
    idx = [_gpu(name, t, torch.int64).reshape(-1).contiguous() for name, t in (("ii", ii), ("jj", jj), ("kk", kk))]
    E = idx[0].numel()
    pay = [_gpu(name, t).reshape(-1, c).contiguous() for name, t, c in (("targets_3d", targets_3d, 3), ("weights", weights, 2),
                                                                       ("weights_pose", weights_pose, 2))]
    if any(t.numel() != E for t in idx) or any(t.shape[0] != E for t in pay):
        raise RuntimeError("prune_keyframe: ii, jj, kk, targets_3d, weights, weights_pose must describe the same E edges")
    Pc, patc, Kc = P.contiguous(), pat.contiguous(), K.contiguous()
    if Kc.shape[0] != Pc.shape[0]:
        raise RuntimeError("prune_keyframe: `intrinsics` must have a row per pose")
    bufs = (_lib.RowBuffer * max(len(frame_buffers), 1))()
    if len(frame_buffers) > 16:
        raise RuntimeError("prune_keyframe: at most 16 frame buffers")
    for b, t in enumerate(frame_buffers):
        _gpu(f"frame_buffers[{b}]", t, None)
        if not t.is_contiguous() or t.dim() < 1 or t.shape[0] < n:
            raise RuntimeError("prune_keyframe: a frame buffer must be contiguous with at least n rows: it is shifted in place")
        bufs[b] = _lib.RowBuffer(t.data_ptr(), t[0].numel() * t.element_size())
    dev = idx[0].device
    L = _lib.lib()
    ws = _ws(dev, E)
    st = torch.cuda.current_stream(dev).cuda_stream
    i64, f32 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.float32, device=dev)
    out = [torch.empty(E, **i64) for _ in range(3)] + [torch.empty(E, 3, **f32), torch.empty(E, 2, **f32), torch.empty(E, 2, **f32)]
    ptr = lambda t: t.data_ptr() if t.numel() else None
    _lib.check(L.bt_keyframe_decide(k, *(ptr(t) for t in idx), E, Pc.data_ptr(), Pc.shape[0], patc.data_ptr(), patc.shape[0],
                                    patc.shape[2] * patc.shape[3], Kc.data_ptr(), float(cfg.beta), float(cfg.KEYFRAME_THRESH),
                                    ws.data_ptr(), st), "bt_keyframe_decide")
    _lib.check(L.bt_edges_prune(k, n, M, int(cfg.REMOVAL_WINDOW), *(ptr(t) for t in idx), *(ptr(t) for t in pay), E,
                                *(ptr(t) for t in out), ws.data_ptr(), st), "bt_edges_prune")
    dP = None
    if k >= 1:                                                  # before the shift moves row k (batrack.py:1042)
        from ..backend.lietorch import SE3
        dP = (SE3(Pc[k:k + 1]) * SE3(Pc[k - 1:k]).inv()).data[0]
    if k >= 0 and len(frame_buffers):
        _lib.check(L.bt_rows_shift(bufs, len(frame_buffers), k, n, ws.data_ptr(), st), "bt_rows_shift")
    host = _host_status(dev)
    host.copy_(ws[:4], non_blocking=True)                       # the call's one read-back
    torch.cuda.current_stream(dev).synchronize()
    s = _lib.KeyframeStatus.from_buffer_copy(host.numpy().tobytes())
    removed, Eo = bool(s.removed), int(s.E_out)
    return KeyframeResult(removed, k, out[0][:Eo], out[1][:Eo], out[2][:Eo], out[3][:Eo][None], out[4][:Eo][None], out[5][:Eo][None],
                          float(s.mag_prev), float(s.mag_next), dP if removed else None)
