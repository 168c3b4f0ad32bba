"""The tracker's `CorrBlock` with the reference's constructor and method signatures
(main/frontend/core/cotracker/blocks.py:326-385), HIP underneath and no correlation volume
(batrack_amd/csrc/corr_lookup.hip through include/batrack_corr.h, which holds the specification).

    fcorr_fn = CorrBlock(fmaps [B,S,C,H,W], num_levels=4, radius=3)     the pyramid, channels-last, once
    fcorr_fn.corr(targets [B,S,N,C])                                    records the targets; nothing is launched
    fcorr_fn.sample(coords [B,S,N,2]) -> [B,S,N,num_levels*(2*radius+1)**2] float32, contiguous

`coords` may be the strided view `coords3[..., :2]` the tracker passes: it is read in place.  Inference only (inputs
are detached, no autograd through the lookup), GPU tensors only; no CPU fallback.

`install()` makes the reference's unmodified tracker use this class: md_tracker.py imports the name `CorrBlock` into its
own namespace, so rebinding it there is all that is needed."""
import importlib

import torch

from .. import _lib


def _gpu(name, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"CorrBlock: `{name}` must be a tensor on the GPU (there is no CPU fallback in batrack_amd)")
    return t.detach().float()


class CorrBlock:
    def __init__(self, fmaps, num_levels=4, radius=4):
        fmaps = _gpu("fmaps", fmaps)
        B, S, C, H, W = fmaps.shape
        self.S, self.C, self.H, self.W = S, C, H, W
        self.B = B
        self.num_levels = num_levels
        self.radius = radius
        self.targets = None
        fm = fmaps.reshape(B * S, C, H, W).contiguous()
        ops = _lib.torch_ops()
        if ops is not None:
            self.pyramid = ops.corr_pyramid(fm, int(num_levels))
        else:
            L = _lib.lib()
            nbytes = L.bt_corr_pyramid_bytes(B * S, C, H, W, int(num_levels))
            self.pyramid = torch.empty(nbytes // 4, dtype=torch.float32, device=fm.device)
            st = torch.cuda.current_stream(fm.device).cuda_stream
            _lib.check(L.bt_corr_pyramid(fm.data_ptr(), B * S, C, H, W, int(num_levels), self.pyramid.data_ptr(), st), "bt_corr_pyramid")

    def sample(self, coords):
        coords = _gpu("coords", coords)
        B, S, N, D = coords.shape
        assert D == 2
        if self.targets is None:
            raise RuntimeError("CorrBlock.sample: call corr(targets) first")
        tg = self.targets
        assert tg.shape[:3] == (B, S, N) and B == self.B
        shape = [B * S, self.C, self.H, self.W]
        ops = _lib.torch_ops()
        if ops is not None:
            return ops.corr_lookup(self.pyramid, shape, int(self.num_levels), int(self.radius), tg, coords)
        d = 2 * self.radius + 1
        out = torch.empty(B, S, N, self.num_levels * d * d, dtype=torch.float32, device=tg.device)
        if N == 0:
            return out
        view = coords.stride(-1) == 1 and coords.stride(-2) >= 2 and B * S * N > 1
        run = coords.stride(-2) * N
        for k in (1, 0):
            view = view and (coords.shape[k] == 1 or coords.stride(k) == run)
            run *= coords.shape[k]
        cd = coords if view else coords.contiguous()
        st = torch.cuda.current_stream(tg.device).cuda_stream
        _lib.check(_lib.lib().bt_corr_lookup(self.pyramid.data_ptr(), *shape, int(self.num_levels), int(self.radius), tg.data_ptr(),
                                             cd.data_ptr(), cd.stride(-2) if view else 2, N, out.data_ptr(), st), "bt_corr_lookup")
        return out

    def corr(self, targets):
        targets = _gpu("targets", targets)
        B, S, N, C = targets.shape
        assert C == self.C
        assert S == self.S
        self.targets = targets.contiguous()


def install(module=None):
    """Rebind the name `CorrBlock` in the reference's tracker module (`main.frontend.md_tracker`, or the module given) to
    the class above; returns the class that was bound before.  Opt-in: nothing in batrack_amd calls it."""
    if module is None:
        module = importlib.import_module("main.frontend.md_tracker")
    previous = getattr(module, "CorrBlock", None)
    module.CorrBlock = CorrBlock
    return previous
