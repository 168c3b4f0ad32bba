"""The feature encoder's stem, trunk and head (the reference's main/frontend/core/cotracker/blocks.py: conv1, norm1, relu1,
the eight `ResidualBlock`s of layer1..4, lines 16-75, and lines 241-273, the last third of `BasicEncoder.forward`, with
norm_fn="instance"), HIP underneath (batrack_amd/csrc/encoder_stem.hip, encoder_trunk.hip and encoder_head.hip through
include/batrack_encoder.h, which holds the specification).

    pack_head_weights(conv2_weight [256,416,3,3], conv3_weight [128,256,1,1]) -> ([52,9,8,256], [256,128])
                                                                                 the layouts the kernels stage (permutations)
    packed_head(conv2, conv3) -> (w2_packed, bias2, w3_packed, bias3)            cached per module pair
    encoder_head(a, b, c, d, conv2, conv3, size, out=None) -> [F,128,h,w]        the four levels resized to `size` (bilinear,
                                                                                 align_corners), concatenated, conv2, instance
                                                                                 norm, ReLU, conv3: neither the resized copies
                                                                                 nor the concatenation is in memory; two launches
    pack_block_weights(conv1_w, conv2_w, down_w=None) -> (w1, w2, wd or None)    [c/8, 9, 8, c_out] twice and [c_in, c_out]
    packed_block(block) -> (w1, b1, w2, b2, wd, bd)                              cached per block; wd, bd None at stride 1
    residual_block(x, block, out=None) -> [F, c_out, ho, wo]                     one residual block: conv, norm, ReLU, conv, norm,
                                                                                 ReLU, (shortcut conv, norm,) add, ReLU; no
                                                                                 normalised map is in memory; five launches
    encoder_trunk(x, layer1, layer2, layer3, layer4) -> (a, b, c, d)             the eight blocks, always on the kernels
    pack_stem_weights(conv1_weight [64,3,7,7]) -> [7,3,8,64]                     w[ky, c, kx, m], the eighth kx a zero
    packed_stem(conv1) -> (w, bias)                                              cached per module
    stem_refusal(enc) -> None or str                                             the first thing that is not the reference's stem
    encoder_stem(x, conv1, out=None) -> [F, 64, ho, wo]                          conv1 7 x 7 stride 2, instance norm, ReLU: the raw
                                                                                 map is written once and normalised in place;
                                                                                 three launches
    forward(self, x)                                                             `BasicEncoder.forward` in our own words: the stem
                                                                                 runs on the kernels when DEVICE_STEM and it is the
                                                                                 reference's (`stem_refusal`), else conv1, norm1,
                                                                                 relu1 are called as they are; a layer in
                                                                                 DEVICE_LAYERS that is a Sequential of residual
                                                                                 blocks runs on the kernels, any other layer is
                                                                                 called as it is; then `encoder_head`

Inference only (no autograd through the kernels), float32, GPU tensors only; no CPU fallback.

`install()` makes the reference's encoder use `forward` from here."""
import ctypes
import importlib
import weakref

import torch

from .. import _lib
from ._conv import KCHUNK, _gpu, bias_of, cached, out_tensor, repack3x3, scratch

LEVELS = (64, 96, 128, 128)  # BT_ENC_CA .. BT_ENC_CD
CIN, CMID, COUT = 416, 256, 128
BLOCK_CHANNELS = (64, 96, 128)
# The layers `forward` sends to the kernels: those whose measured device time is not above torch's at 12 and at 6 frames of
# 64 x 192 x 256 (profiles/r26_encoder_trunk.txt; DESIGN.md f-13 has both numbers of every layer).
DEVICE_LAYERS = ("layer1", "layer2")
CIMG, CSTEM = 3, 64          # BT_ENC_CIMG, BT_ENC_CSTEM
# Whether `forward` sends the stem to the kernels: only if its measured device time is not above torch's at 12 and at 6 frames
# of 3 x 384 x 512 (profiles/r28_encoder_stem.txt).
DEVICE_STEM = True


def _conv_refusal(conv, kernel, padding, strides):
    """None, or what keeps `conv` from being a kernel x kernel Conv2d with that (zero) padding, one of `strides`, a bias, no
    dilation and one group, in words that follow the convolution's name."""
    if not isinstance(conv, torch.nn.Conv2d):
        return f"must be a Conv2d, not {type(conv).__name__}"
    if conv.bias is None:
        return "has no bias"
    if tuple(conv.kernel_size) != (kernel, kernel) or tuple(conv.padding) != (padding, padding) or tuple(conv.stride) not in strides \
            or tuple(conv.dilation) != (1, 1) or conv.groups != 1 or (padding and getattr(conv, "padding_mode", "zeros") != "zeros"):
        return f"must be {kernel} x {kernel} with padding {padding} (zeros), stride {' or '.join(str(s[0]) for s in strides)}, no dilation and one group"
    return None


def _norm_refusal(m):
    """None, or what keeps `m` from being the reference's norm (norm_fn "instance"), in words that follow the norm's name."""
    if not isinstance(m, torch.nn.InstanceNorm2d):
        return f" must be an InstanceNorm2d (norm_fn \"instance\"), not {type(m).__name__}"
    if m.affine or m.track_running_stats or getattr(m, "weight", None) is not None or getattr(m, "running_mean", None) is not None:
        return " must be an InstanceNorm2d without affine parameters or running statistics"
    if abs(float(m.eps) - 1e-5) > 1e-12:
        return f"'s eps must be 1e-5, not {m.eps}"
    return None


def pack_head_weights(conv2_weight, conv3_weight):
    """[256, 416, 3, 3] -> [52, 9, 8, 256]: w2[c // 8, 3 ky + kx, c % 8, m] = conv2_weight[m, c, ky, kx];
    [128, 256, 1, 1] -> [256, 128]: w3[m, o] = conv3_weight[o, m, 0, 0].  Permutations of the weights (any device)."""
    if tuple(conv2_weight.shape) != (CMID, CIN, 3, 3):
        raise RuntimeError(f"encoder_head: conv2 must be 3 x 3 from {CIN} to {CMID} channels, not {tuple(conv2_weight.shape)}")
    if tuple(conv3_weight.shape) != (COUT, CMID, 1, 1):
        raise RuntimeError(f"encoder_head: conv3 must be 1 x 1 from {CMID} to {COUT} channels, not {tuple(conv3_weight.shape)}")
    return repack3x3(conv2_weight), conv3_weight.detach().float().reshape(COUT, CMID).t().contiguous()


_packed = weakref.WeakKeyDictionary()        # conv2 -> (key, the four tensors)


def packed_head(conv2, conv3):
    """The two modules' repacked weights and their biases, redone when any of the four tensors is replaced or written to."""
    for name, conv, kernel, padding in (("conv2", conv2, 3, 1), ("conv3", conv3, 1, 0)):
        why = _conv_refusal(conv, kernel, padding, ((1, 1),))
        if why is not None:
            raise RuntimeError(f"encoder_head: {name} {why}")

    def build():
        w2, w3 = pack_head_weights(conv2.weight, conv3.weight)
        return w2, bias_of(conv2), w3, bias_of(conv3)
    # the partner in the key: a weak reference equals another one only while both name the same living module
    return cached(_packed, conv2, (conv2.weight, conv2.bias, conv3.weight, conv3.bias), build, extra=(weakref.ref(conv3),))


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
    out = out_tensor(out, (F, COUT, h, w), levels[0].device, "encoder_head", f"a contiguous float32 [F, {COUT}, h, w] on the GPU of the maps")
    ops = _lib.torch_ops()
    if ops is not None:
        ops.encoder_head(*levels, w2, b2, w3, b3, out)
        return out
    L = _lib.lib()
    ws = scratch(L.bt_encoder_head_workspace_bytes(F, h, w), out.device, "encoder_head")
    lv = [_level(t) for t in levels]
    _lib.check(L.bt_encoder_head(*(ctypes.byref(v) for v in lv), w2.data_ptr(), b2.data_ptr(), CMID, w3.data_ptr(), b3.data_ptr(), COUT,
                                 F, h, w, ws.data_ptr(), out.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream),
               "bt_encoder_head")
    return out


# ------------------------------------------------------------------------------------------------------ the residual blocks
def pack_block_weights(conv1_w, conv2_w, down_w=None):
    """[c_out, c_in, 3, 3] -> [c_in / 8, 9, 8, c_out]: w1[c // 8, 3 ky + kx, c % 8, m] = conv1_w[m, c, ky, kx]; conv2_w
    [c_out, c_out, 3, 3] likewise; down_w [c_out, c_in, 1, 1] -> [c_in, c_out]: wd[c, m] = down_w[m, c, 0, 0] (None stays None).
    Permutations of the weights (any device)."""
    c_out, c_in = (int(v) for v in conv1_w.shape[:2]) if conv1_w.dim() == 4 else (-1, -1)
    if tuple(conv1_w.shape[2:]) != (3, 3) or c_in not in BLOCK_CHANNELS or c_out not in BLOCK_CHANNELS:
        raise RuntimeError(f"residual_block: conv1 must be 3 x 3 between 64, 96 or 128 channels, not {tuple(conv1_w.shape)}")
    if tuple(conv2_w.shape) != (c_out, c_out, 3, 3):
        raise RuntimeError(f"residual_block: conv2 must be 3 x 3 from {c_out} to {c_out} channels, not {tuple(conv2_w.shape)}")
    if down_w is not None and tuple(down_w.shape) != (c_out, c_in, 1, 1):
        raise RuntimeError(f"residual_block: downsample[0] must be 1 x 1 from {c_in} to {c_out} channels, not {tuple(down_w.shape)}")
    wd = None if down_w is None else down_w.detach().float().reshape(c_out, c_in).t().contiguous()
    return repack3x3(conv1_w), repack3x3(conv2_w), wd


def is_residual_shaped(block):
    """The attributes of a `ResidualBlock`, whatever its class: conv1 and conv2 3 x 3 convolutions, norm1, norm2 and a
    `downsample` attribute.  What `check_block` then refuses is an error, not a reason to leave the layer to torch."""
    return all(isinstance(getattr(block, n, None), torch.nn.Conv2d) and tuple(getattr(block, n).kernel_size) == (3, 3) for n in ("conv1", "conv2")) \
        and hasattr(block, "norm1") and hasattr(block, "norm2") and hasattr(block, "downsample")


def _check_norm(m, name):
    why = _norm_refusal(m)
    if why is not None:
        raise RuntimeError(f"residual_block: {name}{why}")


def check_block(block):
    """Raises, naming what it refuses, unless `block` has the reference's residual shape; returns its stride."""
    if not is_residual_shaped(block):
        raise RuntimeError("residual_block: the block must have conv1, conv2 (3 x 3 convolutions), norm1, norm2 and downsample")
    conv1, conv2 = block.conv1, block.conv2
    if _conv_refusal(conv1, 3, 1, ((1, 1), (2, 2))):
        raise RuntimeError("residual_block: conv1 must be 3 x 3 with padding 1 (zeros), stride 1 or 2, a bias, no dilation and one group")
    if _conv_refusal(conv2, 3, 1, ((1, 1),)):
        raise RuntimeError("residual_block: conv2 must be 3 x 3 with padding 1 (zeros), stride 1, a bias, no dilation and one group")
    stride, c_in, c_out = conv1.stride[0], conv1.in_channels, conv1.out_channels
    if c_in not in BLOCK_CHANNELS or c_out not in BLOCK_CHANNELS or conv2.in_channels != c_out or conv2.out_channels != c_out:
        raise RuntimeError(f"residual_block: channel counts must be 64, 96 or 128 and conv2 square, not {c_in} -> {c_out} -> {conv2.out_channels}")
    _check_norm(block.norm1, "norm1")
    _check_norm(block.norm2, "norm2")
    down = block.downsample
    if stride == 1:
        if down is not None:
            raise RuntimeError("residual_block: a stride-1 block must have downsample None")
        if c_in != c_out:
            raise RuntimeError(f"residual_block: a stride-1 block must keep its channel count, not {c_in} -> {c_out}")
    else:
        if down is None or not isinstance(down, torch.nn.Sequential) or len(down) != 2:
            raise RuntimeError("residual_block: a stride-2 block's downsample must be a Sequential of a convolution and a norm")
        if _conv_refusal(down[0], 1, 0, ((2, 2),)) or down[0].in_channels != c_in or down[0].out_channels != c_out:
            raise RuntimeError(f"residual_block: downsample[0] must be 1 x 1 with stride 2, no padding and a bias, from {c_in} to {c_out} channels")
        _check_norm(down[1], "downsample[1]")
    return stride


_packed_blocks = weakref.WeakKeyDictionary()  # block -> (key, the six tensors)


def packed_block(block):
    """(w1, b1, w2, b2, wd, bd) of a residual block (wd, bd None at stride 1), redone when any tensor is replaced or written to."""
    stride = check_block(block)
    down = block.downsample[0] if stride == 2 else None
    convs = [block.conv1, block.conv2] + ([down] if down is not None else [])

    def build():
        w1, w2, wd = pack_block_weights(block.conv1.weight, block.conv2.weight, None if down is None else down.weight)
        return w1, bias_of(block.conv1), w2, bias_of(block.conv2), wd, None if down is None else bias_of(down)
    return cached(_packed_blocks, block, [t for c in convs for t in (c.weight, c.bias)], build)


def residual_block(x, block, out=None):
    """x [F, c_in, h, w] (any strides, any size >= 1 x 1) through one residual block; `out`, when given, is a contiguous
    [F, c_out, ho, wo] (a slice of a larger buffer), ho = (h - 1) // stride + 1."""
    x = _gpu("x", x, "residual_block")
    w1, b1, w2, b2, wd, bd = packed_block(block)
    stride, c_in, c_out = (2 if wd is not None else 1), w1.shape[0] * KCHUNK, w1.shape[3]
    if x.dim() != 4 or x.shape[1] != c_in or min(x.shape) < 1:
        raise RuntimeError(f"residual_block: `x` must be [F, {c_in}, h, w] and not empty, not {tuple(x.shape)}")
    if not w1.is_cuda or w1.device != x.device:
        raise RuntimeError("residual_block: the block must be on the GPU of `x` (there is no CPU fallback in batrack_amd)")
    F, ho, wo = x.shape[0], (x.shape[2] - 1) // stride + 1, (x.shape[3] - 1) // stride + 1
    out = out_tensor(out, (F, c_out, ho, wo), x.device, "residual_block", f"a contiguous float32 [F, {c_out}, {ho}, {wo}] on the GPU of `x`")
    ops = _lib.torch_ops()
    if ops is not None:
        ops.res_block(x, w1, b1, w2, b2, wd, bd, stride, out)
        return out
    L = _lib.lib()
    ws = scratch(L.bt_res_block_workspace_bytes(F, c_out, x.shape[2], x.shape[3], stride), x.device, "residual_block")
    blk = _lib.ResBlock(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), wd.data_ptr() if stride == 2 else None,
                        bd.data_ptr() if stride == 2 else None, c_in, c_out, stride)
    lx = _level(x)
    _lib.check(L.bt_res_block(ctypes.byref(lx), ctypes.byref(blk), F, ws.data_ptr(), out.data_ptr(),
                              torch.cuda.current_stream(x.device).cuda_stream), "bt_res_block")
    return out


# ---------------------------------------------------------------------------------------------------------------- the stem
def pack_stem_weights(conv1_weight):
    """[64, 3, 7, 7] -> [7, 3, 8, 64]: w[ky, c, kx, m] = conv1_weight[m, c, ky, kx] for kx < 7 and w[ky, c, 7, m] = 0.  A
    permutation of the 9408 weights plus 1344 zeros (any device)."""
    if tuple(conv1_weight.shape) != (CSTEM, CIMG, 7, 7):
        raise RuntimeError(f"encoder_stem: conv1 must be 7 x 7 from {CIMG} to {CSTEM} channels, not {tuple(conv1_weight.shape)}")
    w = conv1_weight.detach().float()
    packed = torch.zeros(7, CIMG, 8, CSTEM, dtype=torch.float32, device=w.device)
    packed[:, :, :7, :] = w.permute(2, 1, 3, 0)
    return packed


def _stem_conv_refusal(conv1):
    why = _conv_refusal(conv1, 7, 3, ((2, 2),))
    if why is not None:                  # a stand-in that is no convolution is named; anything else gets the stem's one sentence
        return "conv1 " + (why if "Conv2d" in why else "must be 7 x 7 with stride 2, padding 3 (zeros), a bias, no dilation and one group")
    if conv1.in_channels != CIMG or conv1.out_channels != CSTEM:
        return f"conv1 must go from {CIMG} to {CSTEM} channels, not {conv1.in_channels} -> {conv1.out_channels}"
    return None


def stem_refusal(enc):
    """None when `enc.conv1`, `enc.norm1`, `enc.relu1` are the reference's stem (what `encoder_stem` computes); otherwise the
    first thing that is not, in words."""
    why = _stem_conv_refusal(getattr(enc, "conv1", None))
    if why is not None:
        return why
    norm1, relu1 = getattr(enc, "norm1", None), getattr(enc, "relu1", None)
    why = _norm_refusal(norm1)
    if why is not None:
        return "norm1" + why
    if not isinstance(relu1, torch.nn.ReLU):
        return f"relu1 must be an nn.ReLU, not {type(relu1).__name__}"
    return None


_packed_stems = weakref.WeakKeyDictionary()   # conv1 -> (key, the two tensors)


def packed_stem(conv1):
    """(w, bias) of the stem's convolution, redone when either tensor is replaced or written to."""
    why = _stem_conv_refusal(conv1)
    if why is not None:
        raise RuntimeError("encoder_stem: " + why)
    return cached(_packed_stems, conv1, (conv1.weight, conv1.bias), lambda: (pack_stem_weights(conv1.weight), bias_of(conv1)))


def encoder_stem(x, conv1, out=None):
    """x [F, 3, h, w] (any strides, any size >= 1 x 1) through conv1, an instance normalisation (eps 1e-5) and a ReLU; `out`,
    when given, is a contiguous [F, 64, ho, wo] (a slice of a larger buffer) that does not overlap x, ho = (h - 1) // 2 + 1."""
    x = _gpu("x", x, "encoder_stem")
    w, b = packed_stem(conv1)
    if x.dim() != 4 or x.shape[1] != CIMG or min(x.shape) < 1:
        raise RuntimeError(f"encoder_stem: `x` must be [F, {CIMG}, h, w] and not empty, not {tuple(x.shape)}")
    if not w.is_cuda or w.device != x.device:
        raise RuntimeError("encoder_stem: conv1 must be on the GPU of `x` (there is no CPU fallback in batrack_amd)")
    F, ho, wo = x.shape[0], (x.shape[2] - 1) // 2 + 1, (x.shape[3] - 1) // 2 + 1
    out = out_tensor(out, (F, CSTEM, ho, wo), x.device, "encoder_stem", f"a contiguous float32 [F, {CSTEM}, {ho}, {wo}] on the GPU of `x`")
    ops = _lib.torch_ops()
    if ops is not None:
        ops.encoder_stem(x, w, b, out)
        return out
    L = _lib.lib()
    ws = scratch(L.bt_encoder_stem_workspace_bytes(F, x.shape[2], x.shape[3]), x.device, "encoder_stem")
    lx = _level(x)
    _lib.check(L.bt_encoder_stem(ctypes.byref(lx), w.data_ptr(), b.data_ptr(), CSTEM, F, ws.data_ptr(), out.data_ptr(),
                                 torch.cuda.current_stream(x.device).cuda_stream), "bt_encoder_stem")
    return out


def is_residual_layer(layer):
    return isinstance(layer, torch.nn.Sequential) and len(layer) > 0 and all(is_residual_shaped(b) for b in layer)


def _run_layer(x, layer):
    for block in layer:
        x = residual_block(x, block)
    return x


def encoder_trunk(x, layer1, layer2, layer3, layer4):
    """x [F, 64, h, w], the stem's output, through the four layers (each a Sequential of residual blocks): (a, b, c, d)."""
    outs = []
    for name, layer in zip(("layer1", "layer2", "layer3", "layer4"), (layer1, layer2, layer3, layer4)):
        if not is_residual_layer(layer):
            raise RuntimeError(f"encoder_trunk: {name} must be a Sequential of residual blocks")
        x = _run_layer(x, layer)
        outs.append(x)
    return tuple(outs)


def forward(self, x):
    if getattr(self, "shallow", False):
        raise RuntimeError("encoder.forward: the shallow encoder (three levels, a 1 x 1 conv2) is not supported")
    if getattr(self, "norm_fn", None) != "instance":
        raise RuntimeError(f"encoder.forward: norm_fn must be \"instance\", not {getattr(self, 'norm_fn', None)!r}")
    why = _norm_refusal(self.norm2)
    if why is not None:
        raise RuntimeError("encoder.forward: norm2" + why)
    if self.training and getattr(self, "dropout", None) is not None:
        raise RuntimeError("encoder.forward: inference only (a training encoder with dropout is not supported)")
    _gpu("x", x, "encoder.forward")
    __, __, H, W = x.shape
    stride = int(self.stride)
    with torch.no_grad():
        x = encoder_stem(x, self.conv1) if DEVICE_STEM and stem_refusal(self) is None else self.relu1(self.norm1(self.conv1(x)))
        maps = []
        for name in ("layer1", "layer2", "layer3", "layer4"):
            layer = getattr(self, name)
            x = _run_layer(x, layer) if name in DEVICE_LAYERS and is_residual_layer(layer) else layer(x)
            maps.append(x)
        return encoder_head(*maps, self.conv2, self.conv3, (H // stride, W // stride))


def install(module=None):
    """Set `BasicEncoder.forward` in the reference's blocks module (`main.frontend.core.cotracker.blocks`, or the module
    given) to `forward` above; returns what was bound before.  Opt-in: nothing in batrack_amd calls it."""
    if module is None:
        module = importlib.import_module("main.frontend.core.cotracker.blocks")
    previous = getattr(module.BasicEncoder, "forward", None)
    module.BasicEncoder.forward = forward
    return previous
