"""Shared by the tests of the tracker's input preparation (include/batrack_video.h, batrack_amd/frontend/video.py), the
fixture generator and the measurement tool: the fixture's cases and their seeded inputs, the stand-ins
`_compute_sparse_tracks` is run on, a torch restatement of the header's arithmetic that computes in the dtype it is given, and
the raw ctypes call."""
import os

import numpy as np
import torch

from track_iter_util import digest                            # noqa: F401  (one copy)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "video_prep.npz")

SIZE = (24, 40)              # the fixture's interp_shape
VEC, TILE, MAX_BLOCKS, GRID_FRAMES = 4, 1024, 1024, 64       # BT_VIDEO_VEC, _TILE, _MAX_BLOCKS, _GRID_FRAMES
# up: 23 x 31 -> 24 x 40, the static mask;  down: 60 x 100 -> 24 x 40, `use_static`;  odd: 61 x 97 -> 24 x 40;  same: the identity
# size, neither.  down's ratio 2.5 is a binary fraction: the reference's float32 and float64 source coordinates are both exact, its
# float64 run can be met to 1e-12, and its gate is arithmetic rounding alone.  odd's ratios are not: the reference's float32
# coordinate makes its gate 1.1e-3, which is what the kernel's exact coordinate is for; and its float64 coordinate's own
# rounding (2e-14 at column 96) times a colour step of up to 255 is 5e-12, so odd is left out of the 1e-12 check (EXACT64) and
# takes part in every other one.
CASES = dict(up=dict(seed=91, T=3, H=23, W=31, N=5, use_static_mask=True, use_static=False),
             down=dict(seed=92, T=3, H=60, W=100, N=4, use_static_mask=False, use_static=True),
             odd=dict(seed=94, T=2, H=61, W=97, N=4, use_static_mask=True, use_static=False),
             same=dict(seed=93, T=2, H=24, W=40, N=3, use_static_mask=False, use_static=False))
RESIZING = ("up", "down", "odd")
EXACT64 = ("up", "down", "same")       # the cases whose float64 run the float64 restatement meets to 1e-12
INPUTS = ("rgbds", "queries")
RETURNS = ("tracks", "depths", "visibilities", "dynamic_e")


def make_inputs(seed, T, H, W, N, **_):
    """Seeded inputs of one case, float32 values in float64 arrays: colours that are integers 0 .. 255, depth in 0.5 .. 20 with
    zeros and values either side of the 0.01 mask, queries (frame, x, y, depth) from inside and just outside the image."""
    rng = np.random.default_rng(seed)
    rgbds = np.concatenate([rng.integers(0, 256, (1, T, 3, H, W)).astype(np.float64), rng.uniform(0.5, 20.0, (1, T, 1, H, W))], 2)
    for t in range(T):
        ys, xs = rng.integers(0, H, 12), rng.integers(0, W, 12)
        rgbds[0, t, 3, ys, xs] = np.resize([0.0, 0.009, 0.011, 0.0099999, 0.0100001, 0.0], 12)
        rgbds[0, t, 3, :2, :3] = 0.0                          # a patch whose resized pixels are exactly zero
    queries = np.stack([rng.integers(0, T, N).astype(np.float64), rng.uniform(-2.0, W + 2.0, N), rng.uniform(-2.0, H + 2.0, N),
                        rng.uniform(0.5, 20.0, N)], -1)[None]
    d = dict(rgbds=rgbds, queries=queries)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in d.items()}


def case_tensors(case, dtype=torch.float32, device="cpu"):
    return {k: torch.as_tensor(v, dtype=dtype, device=device) for k, v in make_inputs(**CASES[case]).items()}


def network_outputs(seed, T, N):
    """What the stand-in network returns (float32 values): its tuple's tensors by name."""
    rng = np.random.default_rng(1000 * seed + 7)
    f = lambda a: a.astype(np.float32)
    return dict(tracks=f(rng.uniform(-4, 44, (1, T, N, 2))), depths=f(rng.uniform(0.5, 20, (1, T, N, 1))),
                static=f(np.concatenate([rng.uniform(-4, 44, (1, T, N, 2)), rng.uniform(0.5, 20, (1, T, N, 1))], -1)),
                visibilities=f(rng.uniform(0, 1, (1, T, N))), dynamic_e=f(rng.uniform(0, 1, (1, T, N))))


class Settings:
    """A settings node with attribute access and `in`."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __contains__(self, k):
        return k in self.__dict__


class StandIn:
    """The plain object `_compute_sparse_tracks` is run on, unbound: the attributes it reads and a recording stand-in
    `network` that returns seeded outputs in the tracker's tuple layout."""

    def __init__(self, case, dtype, device, backward=True, S_slam=12):
        spec = CASES[case]
        self.spec, self.dtype, self.device = spec, dtype, device
        self.interp_shape, self.S_slam = SIZE, S_slam
        self.cfg = Settings(model=Settings(mode="md_tracker", I=4, S=12, use_static_mask=spec["use_static_mask"], use_static=spec["use_static"]),
                            slam=Settings(STATIC_THRESHOLD=0.1, backward_tracking=backward))
        self.seen = []

    def network(self, rgbds, queries, iters):
        self.seen.append(dict(rgbds=rgbds.detach().clone(), queries=queries.detach().clone(), iters=iters))
        o = network_outputs(self.spec["seed"], self.spec["T"], self.spec["N"])
        t = lambda a: torch.as_tensor(a, dtype=self.dtype, device=self.device)
        return t(o["tracks"]), None, t(o["depths"]), t(o["static"]), t(o["visibilities"]), t(o["dynamic_e"]), None


# ------------------------------------------------------------------------------------------------------ the restatement
def taps(n_in, n_out, dtype):
    """(i0, i1, l0, l1) of every output index: the source coordinate max(0, (o + 0.5) n_in / n_out - 0.5) taken exactly in
    integers, its fraction one division in `dtype`."""
    o = torch.arange(n_out, dtype=torch.int64)
    num, den = ((2 * o + 1) * n_in - n_out).clamp(min=0), 2 * n_out
    i0 = num // den
    l1 = (num % den).to(dtype) / torch.tensor(den, dtype=dtype)               # a tensor divisor: a true division
    return i0, i0 + (i0 < n_in - 1).long(), 1 - l1, l1


def resize(x, size):
    """x [..., H, W] -> [..., oh, ow] in x's dtype, on the CPU: ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d), each operation
    rounded (eager torch contracts nothing)."""
    x = x.cpu()
    (y0, y1, ly0, ly1), (x0, x1, lx0, lx1) = taps(x.shape[-2], size[0], x.dtype), taps(x.shape[-1], size[1], x.dtype)
    top, bot = x[..., y0, :], x[..., y1, :]
    row = lambda r: lx0 * r[..., x0] + lx1 * r[..., x1]
    return ly0[:, None] * row(top) + ly1[:, None] * row(bot)


def touched(n_in, n_out, index):
    """Which output indices have the input index among their two taps."""
    i0, i1, __, __ = taps(n_in, n_out, torch.float32)
    return (i0 == index) | (i1 == index)


def normalise(v):
    return 2 * (v / torch.tensor(255.0, dtype=v.dtype)) - 1.0


def depth_process(d, log):
    return torch.log(d.clamp(min=1e-3)) if log else d


def depth_range(plane, log):
    """(min, max) floats of one resized depth plane by the rules of bt_depth_range; (inf, -inf) when nothing is selected."""
    v = depth_process(plane, log)
    if not log:
        v = v[plane > 0.01]
    return (float("inf"), float("-inf")) if v.numel() == 0 else (float(v.min()), float(v.max()))


def compute_sparse_tracks(me, rgbds, queries):
    """`_compute_sparse_tracks` on a StandIn in the dtype of `rgbds`, with `resize` for the interpolation."""
    __, T, __, H, W = rgbds.shape
    oh, ow = me.interp_shape
    queries = queries.clone()
    queries[:, :, 1] *= ow / W
    queries[:, :, 2] *= oh / H
    tracks, __, depths, static, vis, dyn, __ = me.network(rgbds=resize(rgbds[0], (oh, ow))[None], queries=queries, iters=me.cfg.model.I)
    if me.cfg.model.use_static_mask:
        m = dyn > (1 - me.cfg.slam.STATIC_THRESHOLD)
        tracks[m], depths[m] = static[..., :2][m], static[..., 2:][m]
    if me.cfg.model.use_static:
        tracks, depths = static[..., :2], static[..., 2:]
    n = tracks.shape[2]
    fr, col = queries[0, :n, 0].long(), torch.arange(n)
    tracks[0, fr, col] = queries[0, :n, 1:3]
    vis[0, fr, col] = 1.0
    tracks[..., 0] *= W / float(ow)
    tracks[..., 1] *= H / float(oh)
    return tracks, depths, vis, dict(dynamic_e=dyn)


# ------------------------------------------------------------------------------------------------------ the raw ABI call
def raw_frame_prep(image, depth, size, normalise=False, log=False, ws=None, out=None, drange=None):
    """bt_frame_prep through ctypes with the tensors as they lie -> (rc, rgbd, drange, ws).  `ws`: a workspace to reuse (int32
    words; its first 4 * ceil(F / 4) must be zero); a new zeroed one otherwise."""
    from batrack_amd import _lib
    L = _lib.lib()
    F, __, H, W = image.shape
    oh, ow = size
    if out is None:
        out = torch.empty(F, 4, oh, ow, dtype=torch.float32, device=image.device)
    if drange is None:
        drange = torch.empty(F, 2, dtype=torch.float32, device=image.device)
    if ws is None:
        ws = torch.zeros((L.bt_frame_prep_workspace_bytes(F, oh, ow) + 3) // 4, dtype=torch.int32, device=image.device)
    rc = L.bt_frame_prep(image.data_ptr(), int(image.dtype == torch.uint8), *image.stride(), depth.data_ptr(), *depth.stride(), F, H, W, oh, ow,
                         int(normalise), int(log), ws.data_ptr(), out.data_ptr(), drange.data_ptr(),
                         torch.cuda.current_stream(image.device).cuda_stream)
    return rc, out, drange, ws


def blocks(oh, ow):
    """The blocks a frame of oh x ow takes (the grid's x)."""
    return min(MAX_BLOCKS, (oh * ((ow + VEC - 1) // VEC) + 255) // 256)


def workspace_bytes(F, oh, ow):
    return (F + 3) // 4 * 16 + F * blocks(oh, ow) * 8
