"""The encoder-head kernels at their limits (batrack_amd/csrc/encoder_head.hip, include/batrack_encoder.h): repeatability, a
frame alone against the same frame in a batch, `out=` into a slice of a larger buffer, strided source views, a constant
channel of conv2, shapes round the 16 x 8 tile and the 128-pixel block, and a workspace that holds anything on entry.

Tolerances.  No bound is derived from the kernels under test.
  bit-equality   wherever the header promises it: a call against itself, a frame alone against the frame in a batch, strided
                 views against contiguous copies, a dirty workspace against a fresh one; the constant channel's exact zero.
  sums           max |kernel - float64 restatement| <= 2 x max |float32 restatement - float64 restatement| on the same inputs
                 on the same GPU.  A 1 x 1 output has one value per channel: every variance is 0, z is 0 and the output is
                 bias3 exactly (torch's instance_norm refuses that shape, so the formula is the reference there)."""
import numpy as np
import pytest
import torch

import encoder_head_util as U
from batrack_amd import _lib
from test_gpu_encoder_head import raw_call

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.5
SIZE, SIZES = (9, 19), ((18, 37), (9, 19), (5, 10), (3, 5))          # the fixture's s4 layout, its own draw


@pytest.fixture(scope="module")
def encoder():
    from batrack_amd.frontend import encoder
    return encoder


@pytest.fixture(scope="module")
def base(encoder):
    """Inputs on F = 3 frames, their convolutions and the result: computed once, never written to."""
    t = U.random_tensors(95, 3, SIZES, device=DEV)
    conv2, conv3 = U.convs(t)
    out = encoder.encoder_head(*(t[n] for n in U.NAMES), conv2, conv3, SIZE)
    return t, conv2, conv3, out


def test_two_calls_give_equal_bits(encoder, base):
    t, conv2, conv3, out = base
    assert torch.equal(encoder.encoder_head(*(t[n] for n in U.NAMES), conv2, conv3, SIZE), out)
    assert bool(torch.isfinite(out).all())


def test_a_frame_alone_has_the_bits_it_has_in_a_batch(encoder, base):
    t, conv2, conv3, out = base
    for f in range(3):
        alone = encoder.encoder_head(*(t[n][f:f + 1] for n in U.NAMES), conv2, conv3, SIZE)
        assert torch.equal(alone[0], out[f]), f


def test_out_is_written_in_place_and_nothing_else_is(encoder, base):
    t, conv2, conv3, out = base
    big = torch.full((7, U.COUT, *SIZE), SENTINEL, device=DEV)
    ret = encoder.encoder_head(*(t[n] for n in U.NAMES), conv2, conv3, SIZE, out=big[2:5])
    assert ret.data_ptr() == big[2:5].data_ptr()
    assert torch.equal(big[2:5], out)
    assert bool((big[:2] == SENTINEL).all()) and bool((big[5:] == SENTINEL).all())
    with pytest.raises(RuntimeError, match="contiguous"):
        encoder.encoder_head(*(t[n] for n in U.NAMES), conv2, conv3, SIZE, out=big[:3, :, :, ::1].transpose(2, 3))


def test_strided_views_are_read_in_place(encoder, base):
    t, conv2, conv3, out = base
    views = {}
    for n, ch in zip(U.NAMES, U.LEVELS):
        F, __, hl, wl = t[n].shape
        wide = torch.full((F + 2, ch + 5, hl, wl + 3), float("nan"), device=DEV)       # a frame slice, a channel slice, a row stride
        wide[1:F + 1, 3:3 + ch, :, 1:wl + 1] = t[n]
        views[n] = wide[1:F + 1, 3:3 + ch, :, 1:wl + 1]
        assert not views[n].is_contiguous()
    assert torch.equal(encoder.encoder_head(*(views[n] for n in U.NAMES), conv2, conv3, SIZE), out)
    last = [t[n].to(memory_format=torch.channels_last) for n in U.NAMES]            # the channel stride 1, the column stride C
    assert torch.equal(encoder.encoder_head(*last, conv2, conv3, SIZE), out)


def test_a_constant_channel_contributes_nothing(encoder, base):
    """Output channel 77 of conv2 with all-zero weights: y2 = bias2[77] everywhere, the mean is exact, the variance clamps at 0,
    z is exactly 0.  So the result equals, bit for bit, the result with conv3's column 77 zeroed as well — and it is finite."""
    t, conv2, conv3, __ = base
    t = dict(t)
    t["w2"] = t["w2"].clone()
    t["w2"][77] = 0
    t["b2"] = t["b2"].clone()
    t["b2"][77] = 0.3                                             # not a dyadic value: its square is not exact in float32
    c2, c3 = U.convs(t)
    got = encoder.encoder_head(*(t[n] for n in U.NAMES), c2, c3, SIZE)
    assert bool(torch.isfinite(got).all())
    t["w3"] = t["w3"].clone()
    t["w3"][:, 77] = 0
    c2z, c3z = U.convs(t)
    assert torch.equal(got, encoder.encoder_head(*(t[n] for n in U.NAMES), c2z, c3z, SIZE))
    t["w3"][:, 77] = 1e30                                         # z = 0 exactly: even this weight brings nothing (and no NaN)
    c2h, c3h = U.convs(t)
    assert torch.equal(got, encoder.encoder_head(*(t[n] for n in U.NAMES), c2h, c3h, SIZE))


@pytest.mark.parametrize("size", [(8, 16), (16, 8), (9, 17), (17, 9), (1, 1), (11, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_round_the_tile(encoder, size):
    """8 x 16 is exactly one tile (16 wide, 8 tall) and one 128-pixel block; 16 x 8 the same pixels the other way; 9 x 17
    and 17 x 9 one pixel into the next tile each way; 11 x 12 = 132 pixels: four into the second pixel block; 1 x 1."""
    h, w = size
    sizes = ((2 * h, 2 * w + 1), (h, w), ((h + 1) // 2, (w + 1) // 2), ((h + 3) // 4, (w + 3) // 4))
    t = U.random_tensors(96 + h, 2, sizes, device=DEV)
    conv2, conv3 = U.convs(t)
    got = encoder.encoder_head(*(t[n] for n in U.NAMES), conv2, conv3, size)
    if size == (1, 1):                                            # (torch's instance_norm refuses a single spatial element)
        assert torch.equal(got, t["b3"].reshape(1, -1, 1, 1).expand(2, -1, 1, 1))
        return
    with torch.no_grad():
        want32 = U.head(*(t[n] for n in U.INPUTS), size)
        want64 = U.head(*(t[n].double() for n in U.INPUTS), size)
    own = float((want32.double() - want64).abs().max())
    err = float((got.double() - want64).abs().max())
    print(f"{h} x {w}: max |encoder_head - restatement64| {err:.3e}; the float32 restatement's own error {own:.3e}")
    assert 0 < own < 5e-4 and err <= 2 * own


def test_the_workspace_needs_no_initialisation(encoder, base):
    """The header: every byte of the workspace that is read is written first.  A workspace of 0xFF bytes (NaNs as float32 and
    as float64), with 0xFF guard bytes behind it that must stay, against a fresh call."""
    t, conv2, conv3, out = base
    packed = encoder.packed_head(conv2, conv3)
    nbytes = _lib.lib().bt_encoder_head_workspace_bytes(3, *SIZE)
    assert nbytes == 3 * 256 * 171 * 4 + 3 * 4 * 256 * 16 and nbytes % 16 == 0
    buf = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    got = raw_call(t, packed, SIZE, ws=buf)
    assert torch.equal(got, out)
    assert bool((buf[nbytes:] == 0xFF).all())
    got = raw_call(t, packed, SIZE, ws=buf)                       # and again on what the first call left
    assert torch.equal(got, out)
