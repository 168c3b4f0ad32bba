"""The residual-block kernels (csrc/encoder_trunk.hip) at their limits, single blocks: every channel shape the encoder has,
sizes around the 16 x 8 tile at both strides, 1 x 1 maps, a dirty workspace, frames in a batch, `out=` into a slice, strided
input views, a constant channel behind huge weights, and a large bias that tells padding the raw map from padding the
normalised one.  Where a result is compared with arithmetic of another order, the bound is twice the float32 restatement's own
error against its float64 run on the same GPU (tests/encoder_trunk_util.py); every other comparison is bit for bit.

Measured on an MI355X (information, not gates): max |ours - restatement64| beside the float32 restatement's own error
    channel shapes (2 x c x 11 x 19)  64-64/1 2.27e-6 2.20e-6   64-96/2 2.79e-6 3.52e-6   96-96/1 1.93e-6 2.82e-6
                                      96-128/2 2.73e-6 4.22e-6  128-128/1 2.05e-6 3.00e-6  128-128/2 2.56e-6 4.96e-6
    stride 1   8 x 16 1.77e-6 1.89e-6   16 x 8 2.20e-6 2.29e-6   9 x 17 2.17e-6 2.06e-6   17 x 9 2.04e-6 1.77e-6
    stride 2   15 x 31 2.53e-6 2.48e-6   16 x 32 2.44e-6 2.27e-6   17 x 33 2.98e-6 2.22e-6
    bias 50    stride 1 8.94e-6 1.55e-5   stride 2 9.32e-6 1.44e-5
"""
import pytest
import torch

import encoder_trunk_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = sorted({(c_in, c_out, stride) for __, __, c_in, c_out, stride in U.BLOCKS})


@pytest.fixture(scope="module")
def encoder():
    from batrack_amd.frontend import encoder
    return encoder


def make_block(c_in, c_out, stride, seed=151):
    """A residual-shaped block on the GPU with seeded weights (kaiming fan-out scale) and biases uniform in +-0.5."""
    g = torch.Generator().manual_seed(seed)
    b = U.Block(c_in, c_out, stride)
    with torch.no_grad():
        for m in b.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / (m.out_channels * m.kernel_size[0] * m.kernel_size[1])) ** 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
    return b.to(DEV).eval().requires_grad_(False)


def make_x(F, c, h, w, seed=152):
    return torch.randn(F, c, h, w, generator=torch.Generator().manual_seed(seed)).abs().to(DEV)


def restate(b, x):
    """The block by the restatement, in x's dtype."""
    conv = lambda c: (c.weight.to(x.dtype), c.bias.to(x.dtype))
    d = conv(b.downsample[0]) if b.downsample is not None else (None, None)
    with torch.no_grad():
        return U.block(x, *conv(b.conv1), *conv(b.conv2), *d)


def check_against_float64(encoder, b, x, what):
    got = encoder.residual_block(x, b)
    want32, want64 = restate(b, x), restate(b, x.double())
    assert got.shape == want64.shape and got.is_contiguous()
    own = float((want32.double() - want64).abs().max())
    err = float((got.double() - want64).abs().max())
    print(f"{what}: max |ours - restatement64| {err:.3e}; the float32 restatement's own error {own:.3e}")
    assert 0 < own < 5e-4 and err <= 2 * own, (what, err, own)
    return got


@pytest.mark.parametrize("c_in,c_out,stride", SHAPES)
def test_every_channel_shape_of_the_encoder(encoder, c_in, c_out, stride):
    assert len(SHAPES) == 6
    check_against_float64(encoder, make_block(c_in, c_out, stride), make_x(2, c_in, 11, 19), f"{c_in} -> {c_out} stride {stride}")


@pytest.mark.parametrize("stride,size", [(1, (8, 16)), (1, (16, 8)), (1, (9, 17)), (1, (17, 9)), (2, (15, 31)), (2, (16, 32)), (2, (17, 33))])
def test_sizes_around_the_tile(encoder, stride, size):
    b = make_block(64, 64 if stride == 1 else 96, stride)
    got = check_against_float64(encoder, b, make_x(1, 64, *size), f"stride {stride} from {size}")
    assert tuple(got.shape[2:]) == U.out_size(size, stride)
    if stride == 2:
        assert tuple(got.shape[2:]) == {(15, 31): (8, 16), (16, 32): (8, 16), (17, 33): (9, 17)}[size]


def test_one_pixel_maps_are_exact(encoder):
    """On a 1 x 1 map every normalised value is exactly 0 (a constant channel's mean is exact)."""
    g = torch.Generator().manual_seed(153)
    for size in ((2, 2), (1, 1)):
        x = torch.randn(2, 64, *size, generator=g).to(DEV)
        out = encoder.residual_block(x, make_block(64, 96, 2))
        assert out.shape == (2, 96, 1, 1) and torch.equal(out, torch.zeros_like(out))
    x = torch.randn(2, 128, 1, 1, generator=g).to(DEV)
    assert float(x.min()) < 0 < float(x.max())
    assert torch.equal(encoder.residual_block(x, make_block(128, 128, 1)), x.clamp(min=0))


@pytest.mark.parametrize("c_in,c_out,stride", [(64, 64, 1), (96, 128, 2)])
def test_workspace_needs_no_initialisation_and_calls_repeat(encoder, c_in, c_out, stride):
    b, x = make_block(c_in, c_out, stride), make_x(2, c_in, 13, 21)
    packed = encoder.packed_block(b)
    first = U.raw_block(x, packed, ws_fill=0xFF)
    assert torch.isfinite(first).all()
    assert torch.equal(U.raw_block(x, packed, ws_fill=0xFF), first) and torch.equal(U.raw_block(x, packed, ws_fill=0x00), first)
    assert torch.equal(encoder.residual_block(x, b), first)


@pytest.mark.parametrize("c_in,c_out,stride", [(64, 64, 1), (64, 96, 2)])
def test_a_frame_alone_has_the_bits_of_the_frame_in_a_batch(encoder, c_in, c_out, stride):
    b, x = make_block(c_in, c_out, stride), make_x(3, c_in, 10, 23)
    batch = encoder.residual_block(x, b)
    for f in range(3):
        assert torch.equal(encoder.residual_block(x[f:f + 1], b), batch[f:f + 1]), f


@pytest.mark.parametrize("c_in,c_out,stride,size", [(64, 64, 1, (9, 18)), (128, 128, 2, (9, 17)), (96, 96, 1, (8, 16))])
def test_out_into_a_slice_between_sentinels(encoder, c_in, c_out, stride, size):
    b, x = make_block(c_in, c_out, stride), make_x(2, c_in, *size)
    want = encoder.residual_block(x, b)
    buf = torch.full((4, *want.shape[1:]), -7.0, device=DEV)
    assert encoder.residual_block(x, b, out=buf[1:3]) is not None
    assert torch.equal(buf[1:3], want) and bool((buf[0] == -7.0).all()) and bool((buf[3] == -7.0).all())
    with pytest.raises(RuntimeError, match="contiguous"):
        encoder.residual_block(x, b, out=buf[:2, :, :, :-1] if want.shape[3] > 1 else buf[:1])


@pytest.mark.parametrize("c_in,c_out,stride,size", [(64, 64, 1, (12, 20)), (64, 96, 2, (12, 21)), (128, 128, 1, (8, 16))])
def test_strided_input_views_are_read_in_place(encoder, c_in, c_out, stride, size):
    b = make_block(c_in, c_out, stride)
    h, w = size
    big = make_x(2, c_in + 16, h + 3, w + 5)
    views = dict(channels=big[:, 8:8 + c_in, :h, :w], columns=big[:, :c_in, 1:1 + h, 3:3 + w],
                 channels_last=big[:, :c_in, :h, :w].contiguous(memory_format=torch.channels_last),
                 every_other=big[:, :c_in, :h, :w].repeat_interleave(2, dim=3)[:, :, :, ::2])
    for name, v in views.items():
        assert not v.is_contiguous() and v.shape == (2, c_in, h, w), name
        assert torch.equal(encoder.residual_block(v, b), encoder.residual_block(v.contiguous(), b)), name


def test_a_constant_channel_behind_huge_weights_contributes_nothing(encoder):
    """conv1's output channel 5 has zero weights: raw = bias, constant, so its mean is exact and its normalised values are
    exactly 0, whatever conv2 multiplies them by."""
    for c_in, c_out, stride in ((64, 64, 1), (64, 96, 2)):
        b = make_block(c_in, c_out, stride)
        with torch.no_grad():
            b.conv1.weight[5].zero_()
            b.conv2.weight[:, 5].fill_(1e30)
        x = make_x(2, c_in, 10, 19)
        got = encoder.residual_block(x, b)
        assert torch.isfinite(got).all()
        with torch.no_grad():
            b.conv2.weight[:, 5].zero_()
        assert torch.equal(encoder.residual_block(x, b), got)


@pytest.mark.parametrize("c_in,c_out,stride", [(64, 64, 1), (64, 96, 2)])
def test_the_padding_is_of_the_normalised_map(encoder, c_in, c_out, stride):
    """With a bias of 50 on conv1, padding raw1 with zeros (and normalising them to -50 / std, or rectifying after) instead
    of padding the normalised, rectified map would move the border by orders of magnitude."""
    b = make_block(c_in, c_out, stride)
    with torch.no_grad():
        b.conv1.bias.fill_(50.0)
    check_against_float64(encoder, b, make_x(1, c_in, 17, 21), f"bias 50, stride {stride}")
