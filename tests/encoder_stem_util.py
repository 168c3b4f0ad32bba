"""Shared by the encoder-stem tests, the fixture generator and the measurement tool: the fixture's cases and their seeded
inputs, a torch restatement of the stem (the reference's `relu1(norm1(conv1(x)))` with norm_fn "instance" in plain torch
operations) — the CPU specification, and on the GPU the baseline the kernels replace — the weight repack stated element by
element, the raw C ABI route and a minimal encoder-shaped module.  Every function computes in the dtype of the tensors it
is given."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

import encoder_trunk_util as T
from track_iter_util import digest              # noqa: F401  (one copy)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_stem.npz")

CIMG, CSTEM = 3, 64
INPUTS = ("x", "w", "b")
# tiles: 40 x 72 -> 20 x 36: nine 16 x 8 tiles, partial ones on both edges, two frames
# odd:   33 x 47 -> 17 x 24: odd sizes, one row beyond two tiles
# tiny:  7 x 5 -> 4 x 3 = 12 pixels, the minimum the condition allows: every window is mostly padding
CASES = dict(tiles=dict(seed=171, F=2, size=(40, 72)), odd=dict(seed=172, F=1, size=(33, 47)), tiny=dict(seed=173, F=3, size=(7, 5)))
# every STEP-th element of the output is stored; each step is coprime to its case's row length (36, 24, 3)
STEP = dict(tiles=7, odd=5, tiny=1)


def out_size(size):
    return tuple((n - 1) // 2 + 1 for n in size)


def make_inputs(seed, F, size, **_):
    """Seeded inputs of one case: float32 values in float64 arrays.  The images are uniform in +-1 (the tracker's
    2 (rgb / 255) - 1), the weights have the reference's kaiming fan-out scale (std = sqrt(2 / (64 * 49))), the biases are
    uniform in +-0.5."""
    rng = np.random.default_rng(seed)
    d = {"x": rng.uniform(-1.0, 1.0, (F, CIMG, *size)),
         "w": rng.standard_normal((CSTEM, CIMG, 7, 7)) * np.sqrt(2.0 / (CSTEM * 49)),
         "b": rng.uniform(-0.5, 0.5, CSTEM)}
    return {k: v.astype(np.float32).astype(np.float64) for k, v in d.items()}


def case_tensors(case, dtype=torch.float32, device="cpu"):
    d = make_inputs(**CASES[case])
    return {k: torch.as_tensor(v, dtype=dtype, device=device) for k, v in d.items()}


def random_tensors(seed, F, size, dtype=torch.float32, device="cpu"):
    """The same draw for shapes that have no fixture."""
    d = make_inputs(seed, F, size)
    return {k: torch.as_tensor(v, dtype=dtype, device=device) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------------ the restatement
def raw(x, w, b):
    """conv1: 7 x 7, stride 2, zero padding 3 of the image."""
    return Fn.conv2d(x, w, b, stride=2, padding=3)


def stem(x, w, b):
    """`relu1(norm1(conv1(x)))`: InstanceNorm2d is eps 1e-5, biased variance, no affine, the instance's statistics."""
    return Fn.relu(Fn.instance_norm(raw(x, w, b), eps=1e-5))


conditions_hold = T.conditions_hold              # at least 12 pixels; every variance at least 1e-3 of the map's mean (one copy)


def pack_stem_weights(w):
    """The repack stated element by element: p[ky, c, kx, m] = w[m, c, ky, kx] for kx < 7, p[ky, c, 7, m] = 0."""
    p = torch.zeros(7, CIMG, 8, CSTEM, dtype=w.dtype)
    for ky in range(7):
        for c in range(CIMG):
            for kx in range(7):
                p[ky, c, kx] = w[:, c, ky, kx]
    return p


# ------------------------------------------------------------------------------------------------ encoder-shaped modules
def conv1_of(t, device=None):
    """A `conv1` module holding the tensors' weight and bias."""
    conv = nn.Conv2d(CIMG, CSTEM, 7, stride=2, padding=3).to(t["w"].dtype)
    with torch.no_grad():
        conv.weight.copy_(t["w"]); conv.bias.copy_(t["b"])
    return conv.to(device if device is not None else t["w"].device).requires_grad_(False)


class StemEncoder(nn.Module):
    """The three attributes of the reference's stem as `BasicEncoder.__init__` builds them (norm_fn "instance"), seeded."""

    def __init__(self, seed=177, in_channels=CIMG):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.conv1 = nn.Conv2d(in_channels, CSTEM, kernel_size=7, stride=2, padding=3)
        self.norm1 = nn.InstanceNorm2d(CSTEM)
        self.relu1 = nn.ReLU(inplace=True)
        with torch.no_grad():
            self.conv1.weight.copy_(torch.randn(self.conv1.weight.shape, generator=g) * (2.0 / (CSTEM * 49)) ** 0.5)
            self.conv1.bias.copy_(torch.rand(CSTEM, generator=g) - 0.5)
        self.eval().requires_grad_(False)

    def forward(self, x):
        return self.relu1(self.norm1(self.conv1(x)))


# ------------------------------------------------------------------------------------------------------ the raw C ABI
def raw_stem(x, packed, ws_fill=None):
    """bt_encoder_stem through ctypes on the current stream; `packed` = (w, bias)."""
    import ctypes
    from batrack_amd import _lib
    L = _lib.lib()
    w, b = packed
    F, h, wd = x.shape[0], x.shape[2], x.shape[3]
    out = torch.empty(F, CSTEM, *out_size((h, wd)), device=x.device)
    ws = torch.empty((L.bt_encoder_stem_workspace_bytes(F, h, wd) + 7) // 8, dtype=torch.float64, device=x.device)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    lx = _lib.EncoderLevel(x.data_ptr(), *x.shape[1:], *x.stride())
    rc = L.bt_encoder_stem(ctypes.byref(lx), w.data_ptr(), b.data_ptr(), CSTEM, F, ws.data_ptr(), out.data_ptr(),
                           torch.cuda.current_stream(x.device).cuda_stream)
    assert rc == _lib.BT_OK, rc
    return out
