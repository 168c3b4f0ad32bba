"""Shared by the encoder-head tests, the fixture generator and the measurement tool: the fixture's cases and their seeded
inputs, a torch restatement of include/batrack_encoder.h (the reference's blocks.py:241-273 in plain torch operations) — the
CPU specification, and on the GPU the baseline the kernels replace — and a small encoder-shaped module for `forward`.
Every function computes in the dtype of the tensors it is given."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from track_iter_util import digest              # noqa: F401  (one copy)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_head.npz")

LEVELS = (64, 96, 128, 128)
CIN, CMID, COUT = 416, 256, 128
F64_STEP = 8             # the float64 run's output is stored every 8th element
NAMES = ("a", "b", "c", "d")
INPUTS = NAMES + ("w2", "b2", "w3", "b3")

# s4:   the stride-4 layout: `b` has the output's size, partial tiles both ways, two tiles across
# s8:   the stride-8 layout: two levels shrink, one is identical, one grows
# thin: one output row (n_out = 1: scale 0), a 1 x 1 source, three tiles across
CASES = dict(s4=dict(seed=91, F=2, stride=4, size=(9, 19), sizes=((18, 37), (9, 19), (5, 10), (3, 5))),
             s8=dict(seed=92, F=1, stride=8, size=(5, 17), sizes=((20, 67), (10, 34), (5, 17), (3, 9))),
             thin=dict(seed=93, F=3, stride=4, size=(1, 33), sizes=((2, 65), (1, 33), (1, 17), (1, 1))))


def make_inputs(seed, F, sizes, **_):
    """Seeded inputs of one case: float32 values in float64 arrays.  The maps are non-negative, as they are after a ReLU;
    the weights have the reference's kaiming fan-out scale (std = sqrt(2 / (out channels * kernel area))), the biases are
    not zero."""
    rng = np.random.default_rng(seed)
    d = {n: np.abs(rng.standard_normal((F, ch, hl, wl))) for n, ch, (hl, wl) in zip(NAMES, LEVELS, sizes)}
    d["w2"] = rng.standard_normal((CMID, CIN, 3, 3)) * np.sqrt(2.0 / (CMID * 9))
    d["b2"] = rng.uniform(-0.5, 0.5, CMID)
    d["w3"] = rng.standard_normal((COUT, CMID, 1, 1)) * np.sqrt(2.0 / COUT)
    d["b3"] = rng.uniform(-0.5, 0.5, COUT)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in d.items()}


def case_tensors(case, dtype=torch.float32, device="cpu"):
    d = make_inputs(**CASES[case])
    return {k: torch.as_tensor(v, dtype=dtype, device=device) for k, v in d.items()}


def random_tensors(seed, F, sizes, dtype=torch.float32, device="cpu"):
    """The same draw for shapes that have no fixture."""
    d = make_inputs(seed, F, sizes)
    return {k: torch.as_tensor(v, dtype=dtype, device=device) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------------ the restatement
def resize(t, size):
    return Fn.interpolate(t, tuple(size), mode="bilinear", align_corners=True)


def conv2_output(a, b, c, d, w2, b2, size):
    """conv2 over the concatenation of the four resized levels: [F, 256, h, w]."""
    return Fn.conv2d(torch.cat([resize(t, size) for t in (a, b, c, d)], 1), w2, b2, padding=1)


def head(a, b, c, d, w2, b2, w3, b3, size):
    """blocks.py:241-273 after layer4: resize, cat, conv2, InstanceNorm2d(256) (eps 1e-5, biased variance, no affine, the
    instance's statistics), ReLU, conv3."""
    y = conv2_output(a, b, c, d, w2, b2, size)
    return Fn.conv2d(Fn.relu(Fn.instance_norm(y, eps=1e-5)), w3, b3)


def pack_head_weights(w2, w3):
    """The repacks stated element by element: p2[c // 8, 3 ky + kx, c % 8, m] = w2[m, c, ky, kx]; p3[m, o] = w3[o, m, 0, 0]."""
    p2 = torch.zeros(CIN // 8, 9, 8, CMID, dtype=w2.dtype)
    for c in range(CIN):
        p2[c // 8, :, c % 8, :] = w2[:, c].reshape(CMID, 9).t()
    p3 = torch.zeros(CMID, COUT, dtype=w3.dtype)
    for m in range(CMID):
        p3[m] = w3[:, m, 0, 0]
    return p2, p3


def convs(t, device=None):
    """(conv2, conv3) modules holding the tensors' weights and biases."""
    conv2, conv3 = nn.Conv2d(CIN, CMID, 3, padding=1), nn.Conv2d(CMID, COUT, 1)
    conv2, conv3 = conv2.to(t["w2"].dtype), conv3.to(t["w2"].dtype)
    with torch.no_grad():
        conv2.weight.copy_(t["w2"]); conv2.bias.copy_(t["b2"]); conv3.weight.copy_(t["w3"]); conv3.bias.copy_(t["b3"])
    dev = device if device is not None else t["w2"].device
    return conv2.to(dev).requires_grad_(False), conv3.to(dev).requires_grad_(False)


# -------------------------------------------------------------------------------------- an encoder-shaped module for `forward`
class Returns(nn.Module):
    """A stand-in layer that returns the map it holds, whatever it is given."""

    def __init__(self, value):
        super().__init__()
        self.value = value

    def forward(self, x):
        return self.value


class SmallEncoder(nn.Module):
    """The attributes and the module names `BasicEncoder.forward` reads, with one seeded convolution per layer in place of the
    residual blocks: a real network of the encoder's shape (strides 2, 1, 2, 2, 2; 64, 96, 128, 128 channels)."""

    def __init__(self, stride=4, seed=97, norm_fn="instance", dropout=0.0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.stride, self.norm_fn, self.shallow = stride, norm_fn, False
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3)
        self.norm1, self.relu1 = nn.InstanceNorm2d(64), nn.ReLU(inplace=True)
        layer = lambda i, o, s: nn.Sequential(nn.Conv2d(i, o, 3, stride=s, padding=1), nn.InstanceNorm2d(o), nn.ReLU(inplace=True))
        self.layer1, self.layer2, self.layer3, self.layer4 = layer(64, 64, 1), layer(64, 96, 2), layer(96, 128, 2), layer(128, 128, 2)
        self.conv2 = nn.Conv2d(CIN, CMID, 3, padding=1)
        self.norm2, self.relu2 = nn.InstanceNorm2d(CMID), nn.ReLU(inplace=True)
        self.conv3 = nn.Conv2d(CMID, COUT, 1)
        self.dropout = nn.Dropout2d(p=dropout) if dropout > 0 else None
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    fan_out = m.out_channels * m.kernel_size[0] * m.kernel_size[1]
                    m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_out) ** 0.5)
                    m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
        self.eval().requires_grad_(False)


def encoder_forward(m, x):
    """`BasicEncoder.forward` (not shallow, eval) on such a module, every statement a torch operation."""
    H, W = x.shape[-2:]
    x = m.relu1(m.norm1(m.conv1(x)))
    a = m.layer1(x)
    b = m.layer2(a)
    c = m.layer3(b)
    d = m.layer4(c)
    return head(a, b, c, d, m.conv2.weight, m.conv2.bias, m.conv3.weight, m.conv3.bias, (H // m.stride, W // m.stride))
