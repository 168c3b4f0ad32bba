"""Shared by the encoder-trunk tests, the fixture generator and the measurement tool: the fixture's cases and their seeded
inputs, a torch restatement of one residual block and of layer1..4 (the reference's blocks.py:16-75 and 241-244 in plain
torch operations) — the CPU specification, and on the GPU the baseline the kernels replace — and residual-shaped modules
that are not the reference's class.  Every function computes in the dtype of the tensors it is given."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

import encoder_head_util as H
from track_iter_util import digest              # noqa: F401  (one copy)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_trunk.npz")

LAYERS = ("layer1", "layer2", "layer3", "layer4")
LEVELS = ("a", "b", "c", "d")
# (layer, index in the layer, c_in, c_out, stride): `BasicEncoder._make_layer` with dims 64, 96, 128, 128 and strides 1, 2, 2, 2
BLOCKS = (("layer1", 0, 64, 64, 1), ("layer1", 1, 64, 64, 1), ("layer2", 0, 64, 96, 2), ("layer2", 1, 96, 96, 1),
          ("layer3", 0, 96, 128, 2), ("layer3", 1, 128, 128, 1), ("layer4", 0, 128, 128, 2), ("layer4", 1, 128, 128, 1))
LAYER_IN = dict(layer1=64, layer2=64, layer3=96, layer4=128)
# every STEP-th element of a level's output is stored (float64 does not compress: full maps would be 1.5 MB); each step is
# coprime to every row length of its level, so the samples sweep all rows, columns, channels and frames
STEP = dict(a=47, b=19, c=7, d=3)

# even:  several tiles both ways; even and odd stride-2 inputs (20 x 36 -> 10 x 18 -> 5 x 9 -> 3 x 5)
# odd:   odd inputs, the last output's halo passes the edge (17 x 33 -> 9 x 17 -> 5 x 9 -> 3 x 5)
# exact: exact tiles (24 x 32 -> 12 x 16 -> 6 x 8 -> 3 x 4)
CASES = dict(even=dict(seed=131, F=2, size=(20, 36)), odd=dict(seed=132, F=1, size=(17, 33)), exact=dict(seed=133, F=1, size=(24, 32)))


def out_size(size, stride):
    return tuple((n - 1) // stride + 1 for n in size)


def level_sizes(size):
    """The four levels' map sizes from layer1's input size."""
    a = tuple(size)
    b = out_size(a, 2)
    c = out_size(b, 2)
    return a, b, c, out_size(c, 2)


def weight_names():
    names = []
    for layer, i, __, __, stride in BLOCKS:
        names += [f"{layer}.{i}.conv1.weight", f"{layer}.{i}.conv1.bias", f"{layer}.{i}.conv2.weight", f"{layer}.{i}.conv2.bias"]
        if stride == 2:
            names += [f"{layer}.{i}.downsample.0.weight", f"{layer}.{i}.downsample.0.bias"]
    return names


def make_inputs(seed, F, size, **_):
    """Seeded inputs of one case: float32 values in float64 arrays.  `x` [F, 64, h, w] is non-negative, as it is after relu1;
    `in.layerK` is a non-negative input of layer K's shape for the test of that layer alone; the weights have the reference's
    kaiming fan-out scale (std = sqrt(2 / (out channels * kernel area))), the biases are uniform in +-0.5."""
    rng = np.random.default_rng(seed)
    d = {"x": np.abs(rng.standard_normal((F, 64, *size)))}
    for layer, hw in zip(LAYERS[1:], level_sizes(size)[:3]):
        d[f"in.{layer}"] = np.abs(rng.standard_normal((F, LAYER_IN[layer], *hw)))
    for layer, i, c_in, c_out, stride in BLOCKS:
        p = f"{layer}.{i}."
        d[p + "conv1.weight"] = rng.standard_normal((c_out, c_in, 3, 3)) * np.sqrt(2.0 / (c_out * 9))
        d[p + "conv1.bias"] = rng.uniform(-0.5, 0.5, c_out)
        d[p + "conv2.weight"] = rng.standard_normal((c_out, c_out, 3, 3)) * np.sqrt(2.0 / (c_out * 9))
        d[p + "conv2.bias"] = rng.uniform(-0.5, 0.5, c_out)
        if stride == 2:
            d[p + "downsample.0.weight"] = rng.standard_normal((c_out, c_in, 1, 1)) * np.sqrt(2.0 / c_out)
            d[p + "downsample.0.bias"] = rng.uniform(-0.5, 0.5, c_out)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in d.items()}


def layer_input(d, layer):
    """The input of the test of `layer` alone: `x` for layer1, the seeded `in.layerK` otherwise."""
    return d["x"] if layer == "layer1" else d[f"in.{layer}"]


def case_tensors(case, dtype=torch.float32, device="cpu"):
    d = make_inputs(**CASES[case])
    return {k: torch.as_tensor(v, dtype=dtype, device=device) for k, v in d.items()}


def random_tensors(seed, F, size, dtype=torch.float32, device="cpu"):
    d = make_inputs(seed, F, size)
    return {k: torch.as_tensor(v, dtype=dtype, device=device) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------------ the restatement
def block(x, w1, b1, w2, b2, wd=None, bd=None):
    """blocks.py:67-75 with norm_fn "instance": InstanceNorm2d is eps 1e-5, biased variance, no affine, the instance's
    statistics.  The stride is 2 exactly when the shortcut's weights are given."""
    stride = 1 if wd is None else 2
    y = Fn.relu(Fn.instance_norm(Fn.conv2d(x, w1, b1, stride=stride, padding=1), eps=1e-5))
    y = Fn.relu(Fn.instance_norm(Fn.conv2d(y, w2, b2, padding=1), eps=1e-5))
    if wd is not None:
        x = Fn.instance_norm(Fn.conv2d(x, wd, bd, stride=2), eps=1e-5)
    return Fn.relu(x + y)


def block_args(t, layer, i):
    p = f"{layer}.{i}."
    return [t[p + "conv1.weight"], t[p + "conv1.bias"], t[p + "conv2.weight"], t[p + "conv2.bias"],
            t.get(p + "downsample.0.weight"), t.get(p + "downsample.0.bias")]


def layer(x, t, name):
    for i in (0, 1):
        x = block(x, *block_args(t, name, i))
    return x


def trunk(x, t):
    outs = []
    for name in LAYERS:
        x = layer(x, t, name)
        outs.append(x)
    return tuple(outs)


def raw_maps(x, t, name):
    """The inputs of every normalisation of one layer, in order: what the generator's conditions are about."""
    maps = []
    for i in (0, 1):
        w1, b1, w2, b2, wd, bd = block_args(t, name, i)
        stride = 1 if wd is None else 2
        r1 = Fn.conv2d(x, w1, b1, stride=stride, padding=1)
        r2 = Fn.conv2d(Fn.relu(Fn.instance_norm(r1, eps=1e-5)), w2, b2, padding=1)
        maps += [r1, r2] + ([Fn.conv2d(x, wd, bd, stride=2)] if wd is not None else [])
        x = block(x, w1, b1, w2, b2, wd, bd)
    return maps


def conditions_hold(maps):
    """At least 12 pixels in every normalised map, and every (frame, channel) variance at least 1e-3 of its map's mean."""
    for m in maps:
        var = m.double().var(dim=(2, 3), unbiased=False)
        if m.shape[2] * m.shape[3] < 12 or float(var.min()) < 1e-3 * float(var.mean()):
            return False
    return True


def pack_block_weights(w1, w2, wd=None):
    """The repacks stated element by element: p[c // 8, 3 ky + kx, c % 8, m] = w[m, c, ky, kx]; pd[c, m] = wd[m, c, 0, 0]."""
    def pack(w):
        c_out, c_in = w.shape[:2]
        p = torch.zeros(c_in // 8, 9, 8, c_out, dtype=w.dtype)
        for c in range(c_in):
            p[c // 8, :, c % 8, :] = w[:, c].reshape(c_out, 9).t()
        return p
    pd = None
    if wd is not None:
        pd = torch.zeros(wd.shape[1], wd.shape[0], dtype=wd.dtype)
        for c in range(wd.shape[1]):
            pd[c] = wd[:, c, 0, 0]
    return pack(w1), pack(w2), pd


# ---------------------------------------------------------------------------------------------- residual-shaped modules
class Block(nn.Module):
    """The attributes of the reference's `ResidualBlock` with norm_fn "instance", in a class of our own: the kernels'
    front end recognises a block by its shape."""

    def __init__(self, c_in, c_out, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(c_in, c_out, 3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(c_out, c_out, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1, self.norm2 = nn.InstanceNorm2d(c_out), nn.InstanceNorm2d(c_out)
        self.downsample = None
        if stride != 1:
            self.norm3 = nn.InstanceNorm2d(c_out)
            self.downsample = nn.Sequential(nn.Conv2d(c_in, c_out, 1, stride=stride), self.norm3)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


def make_layers(t=None, device=None, dtype=torch.float32):
    """The four layers as Sequentials of two `Block`s; with `t`, holding its weights and biases."""
    layers = {name: [] for name in LAYERS}
    for name, i, c_in, c_out, stride in BLOCKS:
        layers[name].append(Block(c_in, c_out, stride))
    seqs = [nn.Sequential(*layers[name]).to(dtype) for name in LAYERS]
    if t is not None:
        with torch.no_grad():
            for name, seq in zip(LAYERS, seqs):
                for key, p in seq.named_parameters():
                    p.copy_(t[f"{name}.{key}"])
    dev = device if device is not None else (next(iter(t.values())).device if t is not None else "cpu")
    return [s.to(dev).eval().requires_grad_(False) for s in seqs]


def module_tensors(layers):
    """The restatement's dictionary from four layers' parameters."""
    return {f"{name}.{key}": p.detach() for name, seq in zip(LAYERS, layers) for key, p in seq.named_parameters()}


class TrunkEncoder(H.SmallEncoder):
    """`SmallEncoder` with real residual layers: the whole encoder's shape, seeded."""

    def __init__(self, stride=4, seed=137):
        super().__init__(stride=stride, seed=seed)
        t = {k: torch.as_tensor(v, dtype=torch.float32) for k, v in make_inputs(seed, 1, (2, 2)).items()}
        self.layer1, self.layer2, self.layer3, self.layer4 = make_layers(t)
        self.eval().requires_grad_(False)


def encoder_forward(m, x):
    """`BasicEncoder.forward` (not shallow, eval) on such a module, every statement a torch operation."""
    Hh, Ww = x.shape[-2:]
    x = Fn.relu(Fn.instance_norm(Fn.conv2d(x, m.conv1.weight, m.conv1.bias, stride=2, padding=3), eps=1e-5))
    a, b, c, d = trunk(x, module_tensors([m.layer1, m.layer2, m.layer3, m.layer4]))
    return H.head(a, b, c, d, m.conv2.weight, m.conv2.bias, m.conv3.weight, m.conv3.bias, (Hh // m.stride, Ww // m.stride))


# ------------------------------------------------------------------------------------------------------ the raw C ABI
def raw_block(x, packed, ws_fill=None):
    """bt_res_block through ctypes on the current stream; `packed` = (w1, b1, w2, b2, wd, bd)."""
    import ctypes
    from batrack_amd import _lib
    L = _lib.lib()
    w1, b1, w2, b2, wd, bd = packed
    stride, c_in, c_out = (1 if wd is None else 2), w1.shape[0] * 8, w1.shape[3]
    F, h, w = x.shape[0], x.shape[2], x.shape[3]
    out = torch.empty(F, c_out, (h - 1) // stride + 1, (w - 1) // stride + 1, device=x.device)
    ws = torch.empty((L.bt_res_block_workspace_bytes(F, c_out, h, w, stride) + 7) // 8, dtype=torch.float64, device=x.device)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    lx = _lib.EncoderLevel(x.data_ptr(), *x.shape[1:], *x.stride())
    blk = _lib.ResBlock(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), None if wd is None else wd.data_ptr(),
                        None if bd is None else bd.data_ptr(), c_in, c_out, stride)
    rc = L.bt_res_block(ctypes.byref(lx), ctypes.byref(blk), F, ws.data_ptr(), out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream)
    assert rc == _lib.BT_OK, rc
    return out
