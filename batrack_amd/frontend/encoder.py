"""The feature encoder's head (the reference's main/frontend/core/cotracker/blocks.py:241-273, the last third of
`BasicEncoder.forward` with norm_fn="instance"), HIP underneath (batrack_amd/csrc/encoder_head.hip through
include/batrack_encoder.h, which holds the specification).

    pack_head_weights(conv2_weight [256,416,3,3], conv3_weight [128,256,1,1]) -> ([52,9,8,256], [256,128])
                                                                                 the layouts the kernels stage (permutations)
    packed_head(conv2, conv3) -> (w2_packed, bias2, w3_packed, bias3)            cached per module pair
    encoder_head(a, b, c, d, conv2, conv3, size, out=None) -> [F,128,h,w]        the four levels resized to `size` (bilinear,
                                                                                 align_corners), concatenated, conv2, instance
                                                                                 norm, ReLU, conv3: neither the resized copies
                                                                                 nor the concatenation is in memory; two launches
    forward(self, x)                                                             `BasicEncoder.forward` in our own words: conv1,
                                                                                 norm1, relu1 and layer1..4 are called as they
                                                                                 are, then `encoder_head`

Inference only (no autograd through the kernels), float32, GPU tensors only; no CPU fallback.

`install()` makes the reference's encoder use `forward` from here."""
import ctypes
import importlib
import weakref

import torch

from .. import _lib

LEVELS = (64, 96, 128, 128)  # BT_ENC_CA .. BT_ENC_CD
CIN, CMID, COUT = 416, 256, 128
KCHUNK = 8                   # BT_WINDOW_KCHUNK


def _gpu(name, t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: `{name}` must be a tensor on the GPU (there is no CPU fallback in batrack_amd)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what}: `{name}` must be float32")
    return t.detach()


def pack_head_weights(conv2_weight, conv3_weight):
    """[256, 416, 3, 3] -> [52, 9, 8, 256]: w2[c // 8, 3 ky + kx, c % 8, m] = conv2_weight[m, c, ky, kx];
    [128, 256, 1, 1] -> [256, 128]: w3[m, o] = conv3_weight[o, m, 0, 0].  Permutations of the weights (any device)."""
    if tuple(conv2_weight.shape) != (CMID, CIN, 3, 3):
        raise RuntimeError(f"encoder_head: conv2 must be 3 x 3 from {CIN} to {CMID} channels, not {tuple(conv2_weight.shape)}")
    if tuple(conv3_weight.shape) != (COUT, CMID, 1, 1):
        raise RuntimeError(f"encoder_head: conv3 must be 1 x 1 from {CMID} to {COUT} channels, not {tuple(conv3_weight.shape)}")
    w2 = conv2_weight.detach().float().permute(1, 2, 3, 0).reshape(CIN // KCHUNK, KCHUNK, 9, CMID).permute(0, 2, 1, 3).contiguous()
    w3 = conv3_weight.detach().float().reshape(COUT, CMID).t().contiguous()
    return w2, w3


_packed = weakref.WeakKeyDictionary()        # conv2 -> (key, conv3 weak reference, the four tensors)


def _check_conv(conv, name, kernel, padding):
    if conv.bias is None:
        raise RuntimeError(f"encoder_head: {name} has no bias")
    if tuple(conv.kernel_size) != (kernel, kernel) or tuple(conv.padding) != (padding, padding) or tuple(conv.stride) != (1, 1) \
            or tuple(conv.dilation) != (1, 1) or conv.groups != 1 or (padding and getattr(conv, "padding_mode", "zeros") != "zeros"):
        raise RuntimeError(f"encoder_head: {name} must be {kernel} x {kernel} with padding {padding} (zeros), stride 1, no dilation and one group")


def packed_head(conv2, conv3):
    """The two modules' repacked weights and their biases, redone when any of the four tensors is replaced or written to."""
    _check_conv(conv2, "conv2", 3, 1)
    _check_conv(conv3, "conv3", 1, 0)
    ts = (conv2.weight, conv2.bias, conv3.weight, conv3.bias)
    key = tuple(v for t in ts for v in (t.data_ptr(), t._version)) + (str(conv2.weight.device),)
    hit = _packed.get(conv2)
    if hit is None or hit[0] != key or hit[1]() is not conv3:
        w2, w3 = pack_head_weights(conv2.weight, conv3.weight)
        hit = (key, weakref.ref(conv3), (w2, conv2.bias.detach().float().contiguous(), w3, conv3.bias.detach().float().contiguous()))
        _packed[conv2] = hit
    return hit[2]


def _level(t):
    return _lib.EncoderLevel(t.data_ptr(), *t.shape[1:], *t.stride())


def encoder_head(a, b, c, d, conv2, conv3, size, out=None):
    """a, b, c, d [F, 64 / 96 / 128 / 128, h_l, w_l] (any strides, any sizes >= 1 x 1) are `layer1..4`'s outputs; `size` =
    (h, w) is the output map's; `out`, when given, is a contiguous [F, 128, h, w] (a slice of a larger buffer)."""
    levels = [_gpu(n, t, "encoder_head") for n, t in zip("abcd", (a, b, c, d))]
    h, w = (int(v) for v in size)
    F = levels[0].shape[0] if levels[0].dim() == 4 else -1
    for n, t, ch in zip("abcd", levels, LEVELS):
        if t.dim() != 4 or t.shape[0] != F or t.shape[1] != ch or t.shape[2] < 1 or t.shape[3] < 1 or t.device != levels[0].device:
            raise RuntimeError(f"encoder_head: `{n}` must be [F, {ch}, h_l, w_l] on the GPU of `a`, not {tuple(t.shape)}")
    if F < 1 or h < 1 or w < 1:
        raise RuntimeError("encoder_head: F, h and w must be at least 1")
    w2, b2, w3, b3 = packed_head(conv2, conv3)
    if not w2.is_cuda or w2.device != levels[0].device or w3.device != w2.device:
        raise RuntimeError("encoder_head: the convolutions must be on the GPU of the maps (there is no CPU fallback in batrack_amd)")
    if out is None:
        out = torch.empty(F, COUT, h, w, dtype=torch.float32, device=levels[0].device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
              and tuple(out.shape) == (F, COUT, h, w) and out.device == levels[0].device):
        raise RuntimeError(f"encoder_head: `out` must be a contiguous float32 [F, {COUT}, h, w] on the GPU of the maps")
    ops = _lib.torch_ops()
    if ops is not None:
        ops.encoder_head(*levels, w2, b2, w3, b3, out)
        return out
    L = _lib.lib()
    nbytes = L.bt_encoder_head_workspace_bytes(F, h, w)
    if nbytes == 0:
        raise RuntimeError("encoder_head: " + _lib.ERRORS[_lib.BT_EUNSUPPORTED])
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=out.device)         # needs no initialisation
    lv = [_level(t) for t in levels]
    _lib.check(L.bt_encoder_head(*(ctypes.byref(v) for v in lv), w2.data_ptr(), b2.data_ptr(), CMID, w3.data_ptr(), b3.data_ptr(), COUT,
                                 F, h, w, ws.data_ptr(), out.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream),
               "bt_encoder_head")
    return out


def _plain_instance_norm(m):
    return isinstance(m, torch.nn.InstanceNorm2d) and not m.affine and not m.track_running_stats \
        and getattr(m, "weight", None) is None and getattr(m, "running_mean", None) is None


def forward(self, x):
    if getattr(self, "shallow", False):
        raise RuntimeError("encoder.forward: the shallow encoder (three levels, a 1 x 1 conv2) is not supported")
    if getattr(self, "norm_fn", None) != "instance":
        raise RuntimeError(f"encoder.forward: norm_fn must be \"instance\", not {getattr(self, 'norm_fn', None)!r}")
    if not _plain_instance_norm(self.norm2):
        raise RuntimeError("encoder.forward: norm2 must be an InstanceNorm2d without affine parameters or running statistics")
    if abs(float(self.norm2.eps) - 1e-5) > 1e-12:
        raise RuntimeError(f"encoder.forward: norm2's eps must be 1e-5, not {self.norm2.eps}")
    if self.training and getattr(self, "dropout", None) is not None:
        raise RuntimeError("encoder.forward: inference only (a training encoder with dropout is not supported)")
    _gpu("x", x, "encoder.forward")
    __, __, H, W = x.shape
    stride = int(self.stride)
    with torch.no_grad():
        x = self.relu1(self.norm1(self.conv1(x)))
        a = self.layer1(x)
        b = self.layer2(a)
        c = self.layer3(b)
        d = self.layer4(c)
        return encoder_head(a, b, c, d, self.conv2, self.conv3, (H // stride, W // stride))


def install(module=None):
    """Set `BasicEncoder.forward` in the reference's blocks module (`main.frontend.core.cotracker.blocks`, or the module
    given) to `forward` above; returns what was bound before.  Opt-in: nothing in batrack_amd calls it."""
    if module is None:
        module = importlib.import_module("main.frontend.core.cotracker.blocks")
    previous = getattr(module.BasicEncoder, "forward", None)
    module.BasicEncoder.forward = forward
    return previous
