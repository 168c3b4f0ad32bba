"""The tracker-window kernels at their limits (batrack_amd/csrc/window_fmaps.hip, include/batrack_window.h): the two-stage
min / max of k_depth_range and k_window_depth on ONE workspace that is never zeroed again (1 element to 1026 blocks wanted,
the extreme and a NaN moved through the blocks and the trips), the selection mask at 0.01, k_window_depth's strides and
padding frames, k_embed_conv's (tap, channel, output column) mapping pinned exactly by one-hot weights, its shapes round the
16 x 8 tile, the reach of a non-finite value, k_feat_sample at 1-row maps, far coordinates, every frame clamp and past its
grid cap, and guard rows round every buffer of the four raw entry points.

Tolerances.  No bound is derived from the kernel under test.
  bit-equality   wherever the header promises it: depth_range and window_depth without log, feat_sample, and the one-hot
                 convolution on the encoder's channels and on the normalised (x, y, z) (every product is x * 1 or x * 0, every
                 partial sum exact, so the result is fl(input + bias)); a frame alone against the same frame in a window;
                 strided inputs against contiguous ones.  The references are the restatement of tests/tracker_window_util.py
                 on the CPU.
  sums           max |kernel - float64 restatement| <= 2 x max |float32 restatement - float64 restatement| on the same
                 inputs, pooled over all calls of a parametrised case (Pool): a 2 x 2 map alone has too few values.
  log form       the device's logf and the host's are each within 1 ulp of the logarithm (|log d| < 8: an ulp of 4.8e-7);
                 the two differ by 2 ulps at most, times Dz / d_range, and the three rounded operations after it add 1.5 ulps
                 of the result (the argument of test_log_depth_range_and_window_depth).
  sine, cosine   a single device sine or cosine: 4 x 2^-24 absolute against float64 at the same float32 argument
                 fl(p * freq) (the allowance test_sine_at_the_float32_argument grants), and half an ulp of the result for
                 the bias add.

Measured on an MI355X (information, not gates):
    one-hot weights, max |sine or cosine channel - float64 at the float32 argument|, bias add included:
        9 x 17   1.653e-07     16 x 33   1.684e-07     the smallest bound of an element 2.384e-07
    shapes round the tile, max |kernel - float64| beside its gate, the float32 restatement's own error (asserted: <= 2 x):
        2 x 2    9.471e-06  8.696e-06      2 x 17   2.221e-05  2.388e-05      9 x 2    2.661e-05  2.661e-05
        8 x 16   4.096e-05  4.203e-05      9 x 16   3.811e-05  3.795e-05      8 x 17   4.255e-05  4.208e-05
        7 x 15   3.833e-05  3.786e-05      17 x 33  3.106e-05  3.166e-05
    log clamp: max |window_depth - float64 restatement| 2.427e-06, bound 4.606e-06
    log range: max |depth_range - float32 restatement| 4.768e-07 at all three sizes, bound 9.600e-07.  The device's logf is
        1.30 ulps from the logarithm at 1e-3f (-6.9077559, one float32 below the host's correctly rounded -6.9077554) and
        0.26, 1.16 and 1.46 ulps at the three maxima near 20: inside the 2 ulps allowed between device and host, outside
        the 1 ulp that argument grants each side."""
import numpy as np
import pytest
import torch

import tracker_window_util as U
from batrack_amd import _lib
from test_gpu_track_iter_limits import GUARD, SENTINEL, Pool, guarded, same_values, stream, untouched
from test_gpu_tracker_window import conv_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNIT = 2.0 ** -24
NAN, INF = float("nan"), float("inf")
F32_MAX = float(np.finfo(np.float32).max)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
WD_THREADS, WD_BLOCK, WD_MAX_BLOCKS = 256, 2048, 1024           # k_depth_range's launch: 256 threads, 8 elements a thread


@pytest.fixture(scope="module")
def tracker():
    from batrack_amd.frontend import tracker
    return tracker


# ------------------------------------------------------------------------------------ 1. the reduction and its ticket
class Workspace:
    """ONE workspace for a whole sequence of raw calls: the partials start as NaN (an unwritten slot that is read would
    show), only the ticket — the last word — is zero, and nothing here ever zeroes it again.  64 sentinel bytes follow."""
    TAIL = 0x5A5A5A5A

    def __init__(self):
        self.words = (_lib.lib().bt_window_workspace_bytes() + 3) // 4
        assert self.words == 2 * WD_MAX_BLOCKS + 1
        self.buf = torch.full((self.words + 16,), self.TAIL, dtype=torch.int32, device=DEV)
        self.buf[:self.words - 1].view(torch.float32).fill_(NAN)
        self.buf[self.words - 1] = 0
        self.calls = 0

    def settle(self):
        """After a call: the ticket reads 0 again and the bytes after the workspace are as they were."""
        torch.cuda.synchronize()
        self.calls += 1
        tail = self.buf[self.words - 1:].cpu()
        assert int(tail[0]) == 0, f"the ticket reads {int(tail[0])} after call {self.calls}"
        assert bool((tail[1:] == self.TAIL).all()), f"call {self.calls} wrote past the workspace"


def raw_depth_range(ws, depth, log=False):
    out = torch.full((2,), SENTINEL, device=DEV)
    rc = _lib.lib().bt_depth_range(depth.data_ptr(), *depth.shape, *depth.stride(), int(log), ws.buf.data_ptr(), out.data_ptr(), stream())
    assert rc == _lib.BT_OK
    ws.settle()
    return out.cpu()


def raw_window_depth(ws, depth, S, stride, d_near, d_far, Dz, log=False):
    h, w = depth.shape[1] // stride, depth.shape[2] // stride
    dm, zr = torch.full((S, h, w), SENTINEL, device=DEV), torch.full((2,), SENTINEL, device=DEV)
    rc = _lib.lib().bt_window_depth(depth.data_ptr(), depth.shape[0], S, depth.shape[1], depth.shape[2], *depth.stride(), stride,
                                    float(d_near), float(d_far) - float(d_near), float(Dz), int(log), ws.buf.data_ptr(), dm.data_ptr(),
                                    zr.data_ptr(), stream())
    assert rc == _lib.BT_OK
    ws.settle()
    return dm, zr.cpu()


def depth_of(T, H, W, seed):
    """Depths in [0.5, 20), a few below the 0.01 mask, float32 values on the CPU."""
    g = torch.Generator().manual_seed(seed)
    d = torch.rand(T, H, W, generator=g) * 19.5 + 0.5
    d.view(-1)[::97] = 0.0
    return d


def pair(lo, hi):
    return torch.stack([torch.as_tensor(lo, dtype=torch.float32).reshape(()), torch.as_tensor(hi, dtype=torch.float32).reshape(())])


SHAPES = {1: (1, 1, 1), 2048: (1, 32, 64), 2049: (3, 1, 683), 529200: (3, 420, 420), 2099520: (5, 648, 648)}
SEQUENCE = [2099520, 1, 529200, 2048, 2049, 2099520, 1, 2049, 529200, 2048, 2099520]        # large -> small -> large, twice


def blocks_of(total):
    return min(WD_MAX_BLOCKS, (total + WD_BLOCK - 1) // WD_BLOCK)


def test_one_workspace_serves_every_size_in_turn():
    """Both entry points alternate over 1, 2048, 2049, 529200 (259 blocks) and 2099520 elements (1026 blocks wanted, 1024
    launched) on one workspace: after a 1024-block launch the partials of the blocks a smaller launch does not have are
    stale, and must not be read; after every call the ticket is zero.  Results: torch's on the CPU copy, bit for bit."""
    assert [blocks_of(n) for n in (1, 2048, 2049, 529200, 2099520)] == [1, 1, 2, 259, 1024]
    assert 2099520 > 8 * WD_MAX_BLOCKS * WD_THREADS and (2099520 + WD_BLOCK - 1) // WD_BLOCK == 1026       # a ninth, ragged trip
    ws = Workspace()
    host = {n: depth_of(*SHAPES[n], 100 + i) for i, n in enumerate(SHAPES)}
    host[1][0, 0, 0] = 7.25                                      # the single element is selected
    dev = {n: d.to(DEV) for n, d in host.items()}
    for i, n in enumerate(SEQUENCE):
        T, H, W = SHAPES[n]
        if i % 2 == 0:
            got = raw_depth_range(ws, dev[n])
            assert torch.equal(got, pair(*U.depth_range(host[n], False))), (i, n)
        d_near, d_far = U.depth_range(host[n], False) if n > 1 else (0.5, 20.0)
        dm, zr = raw_window_depth(ws, dev[n], T, 1, d_near, d_far, W)
        want, __ = U.window_depth(host[n], T, 1, d_near, d_far, W, False)
        assert torch.equal(dm.cpu(), want) and torch.equal(zr, pair(want.min(), want.max())), (i, n)
        if i % 2 == 1:
            got = raw_depth_range(ws, dev[n])
            assert torch.equal(got, pair(*U.depth_range(host[n], False))), (i, n)
    # the log form in the same workspace: the unmasked range, within 2 ulps (|log| < 8) of the float32 restatement's
    for n in (529200, 2049, 2099520):
        got = raw_depth_range(ws, dev[n], log=True).double()
        want = torch.tensor(U.depth_range(host[n], True), dtype=torch.float64)
        truth = torch.tensor(U.depth_range(host[n].clamp(min=1e-3).double(), True), dtype=torch.float64)
        ulps = (got - truth).abs() / torch.from_numpy(np.spacing(truth.abs().numpy().astype(np.float32))).double()
        print(f"log range, {n} elements: max |depth_range - float32 restatement| {float((got - want).abs().max()):.3e}, bound {2 * 4.8e-7:.3e}; "
              f"the device's (min, max) are ({ulps[0]:.2f}, {ulps[1]:.2f}) ulps from the logarithm")
        assert want[0] < -6.9 and float((got - want).abs().max()) <= 2 * 4.8e-7, n
    assert ws.calls == 2 * len(SEQUENCE) + 3


def positions(total):
    """Where an extreme can be lost: the first lanes and waves, the ends of a thread's and a block's first share, the first
    element of blocks 255, 256 and 257 and of the last block (block b's first trip starts at 256 b; were the blocks
    contiguous shares of 2048 it would be 2048 b: both), and the last element, which is in the last, ragged trip."""
    nb = blocks_of(total)
    pos = [0, 63, 64, 255, 256, 2047, 2048]
    for b in (255, 256, 257, nb - 1):
        pos += [WD_THREADS * b, WD_BLOCK * b]
    pos += [total - 1]
    return sorted({p for p in pos if 0 <= p < total})


@pytest.mark.parametrize("total", [529200, 2099520])
def test_an_extreme_anywhere_reaches_the_result(total):
    """All values strictly inside (2, 9); the minimum 1.5, then the maximum 9.5, then a NaN (log form) at each position,
    one call each, on one workspace.  With d_near = 0, d_range = 1 and Dz = 1 the depth maps are the depths themselves."""
    T, H, W = SHAPES[total]
    g = torch.Generator().manual_seed(total)
    base = (torch.rand(T, H, W, generator=g) * 6.5 + 2.25).to(DEV)
    lo, hi = float(base.min()), float(base.max())
    assert 2.0 < lo and hi < 9.0
    ws = Workspace()
    pos = positions(total)
    assert total - 1 in pos and WD_THREADS * 256 in pos and WD_THREADS * (blocks_of(total) - 1) in pos
    for p in pos:
        for value, want in ((1.5, (1.5, hi)), (9.5, (lo, 9.5))):
            d = base.clone()
            d.view(-1)[p] = value
            assert (float(d.min()), float(d.max())) == want
            assert torch.equal(raw_depth_range(ws, d), pair(*want)), (p, value)
            dm, zr = raw_window_depth(ws, d, T, 1, 0.0, 1.0, 1.0)
            assert torch.equal(zr, pair(*want)) and torch.equal(dm, d), (p, value)
        d = base.clone()
        d.view(-1)[p] = NAN
        assert bool(torch.isnan(raw_depth_range(ws, d, log=True)).all()), p
        dm, zr = raw_window_depth(ws, d, T, 1, 0.0, 1.0, 1.0, log=True)
        assert bool(torch.isnan(zr).all()) and int(torch.isnan(dm).sum()) == 1, p
        assert torch.equal(raw_depth_range(ws, d), pair(lo, hi)), p           # the mask does not select a NaN
    assert torch.equal(raw_depth_range(ws, base), pair(lo, hi))


def test_the_mask_at_its_boundary(tracker):
    """d > 0.01 in float32: 0.01f itself is not selected, its successor is.  Nothing selected: exactly (+inf, -inf), and
    the front end's error."""
    c = np.float32(0.01)
    below, above = np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(1))
    v = torch.tensor([below, c, above, 0.0, -0.0, 1e-40, -3.0, INF], dtype=torch.float32)
    sel = v[v > 0.01]
    assert sel.tolist() == [float(above), INF]                   # what torch selects on the CPU
    ws = Workspace()
    for n in (8, 7, 3, 2):                                       # with +inf, without it, up to the successor, up to 0.01f
        d = v[:n].reshape(1, 1, n)
        s = d[d > 0.01]
        want = pair(s.min(), s.max()) if s.numel() else pair(INF, -INF)
        assert torch.equal(raw_depth_range(ws, d.to(DEV)), want), n
    assert torch.equal(raw_depth_range(ws, v[:2].reshape(1, 2, 1).to(DEV)), pair(INF, -INF))
    none = torch.full((3, 50, 41), float(c), device=DEV)
    none[1, 7, 5], none[2, 49, 40] = -2.0, 0.0
    assert torch.equal(raw_depth_range(ws, none), pair(INF, -INF))
    assert torch.equal(tracker.depth_range(none).cpu(), pair(INF, -INF))
    none[0, 0, 0] = float(above)
    assert torch.equal(tracker.depth_range(none).cpu(), pair(above, above))
    me = U.StandIn("C", torch.float32, DEV, U.embed3d_stand_in())
    T = U.case_tensors("C", device=DEV)
    T["rgbds"][0, :, 3] = float(c)
    with pytest.raises(RuntimeError, match="no depth above 0.01"):
        tracker.forward(me, T["rgbds"], T["queries"])
    assert me.fnet_calls == 0


def test_depth_views_are_read_in_place(tracker):
    """stride_x != 1 (a transposed view), stride_t == 0 (one frame expanded to T) and the channel view, through the front
    end and through the raw entry points: torch's results on the CPU copy of the same view."""
    g = torch.Generator().manual_seed(7)
    T, H, W, stride = 3, 39, 69, 4
    views = {"transposed": (torch.rand(T, W, H, generator=g) * 19.5 + 0.5).to(DEV).transpose(1, 2),
             "expanded": (torch.rand(1, H, W, generator=g) * 19.5 + 0.5).to(DEV).expand(T, H, W),
             "channel": (torch.rand(T, 4, H, W, generator=g) * 19.5 + 0.5).to(DEV)[:, 3]}
    assert views["transposed"].stride(2) == H and views["expanded"].stride(0) == 0 and views["channel"].stride(0) == 4 * H * W
    ws = Workspace()
    for name, d in views.items():
        d[0, 5, 9] = 0.0                                         # below the mask
        host = d.cpu()
        want = pair(*U.depth_range(host, False))
        assert torch.equal(tracker.depth_range(d).cpu(), want) and torch.equal(raw_depth_range(ws, d), want), name
        for S in (T, T + 2):
            dm_want, zr_want = U.window_depth(host, S, stride, 0.5, 20.0, W // stride, False)
            dm, zr = tracker.window_depth(d, S, stride, 0.5, 20.0, W // stride)
            assert torch.equal(dm.cpu(), dm_want) and torch.equal(zr.cpu(), pair(*zr_want)), (name, S)
            dm, zr = raw_window_depth(ws, d, S, stride, 0.5, 20.0, W // stride)
            assert torch.equal(dm.cpu(), dm_want) and torch.equal(zr, pair(*zr_want)), (name, S)


# ------------------------------------------------------------------------------------------- 2. window_depth shapes
@pytest.mark.parametrize("stride", [1, 2, 8])
def test_window_depth_shapes(tracker, stride):
    """H = 8 h + 7 and W = 8 w + 5 (no multiples of the stride but for stride 1), a 1 x 1 map, one frame padded to S = 8,
    frames = S: bit-equal to the float32 restatement on the CPU."""
    g = torch.Generator().manual_seed(20 + stride)
    for frames, S, H, W in ((3, 4, 8 * 3 + 7, 8 * 5 + 5), (1, 8, 8 * 2 + 7, 8 * 3 + 5), (4, 4, 8 * 1 + 7, 8 * 9 + 5), (2, 3, stride, stride),
                            (1, 1, stride, 2 * stride + (stride > 1))):
        host = torch.rand(frames, H, W, generator=g) * 19.5 + 0.5
        want, zr_want = U.window_depth(host, S, stride, 0.5, 20.0, W // stride, False)
        dm, zr = tracker.window_depth(host.to(DEV), S, stride, 0.5, 20.0, W // stride)
        assert dm.shape == (S, H // stride, W // stride) == want.shape
        assert torch.equal(dm.cpu(), want) and torch.equal(zr.cpu(), pair(*zr_want)), (frames, S, H, W)
        if frames < S:                                           # every padding frame repeats the last one, and zrange covers them
            assert all(torch.equal(dm[t], dm[frames - 1]) for t in range(frames, S))


@pytest.mark.parametrize("stride", [2, 8])
def test_window_depth_reads_the_lattice_only(tracker, stride):
    """A NaN and an inf OFF the stride lattice change nothing; ON it a NaN gives one NaN in dmaps — one per copy when it
    is in the last frame of a short window — and a NaN zrange; an inf gives the restatement's result."""
    frames, S, H, W = 2, 4, 8 * 3 + 7, 8 * 4 + 5
    g = torch.Generator().manual_seed(30 + stride)
    host = torch.rand(frames, H, W, generator=g) * 19.5 + 0.5
    clean = tracker.window_depth(host.to(DEV), S, stride, 0.5, 20.0, W // stride)
    for bad in (NAN, INF):
        off = host.clone()
        off[0, stride + 1, 2 * stride], off[1, 2 * stride, stride - 1], off[1, H - 1, W - 1] = bad, bad, bad
        dm, zr = tracker.window_depth(off.to(DEV), S, stride, 0.5, 20.0, W // stride)
        assert torch.equal(dm, clean[0]) and torch.equal(zr, clean[1]), bad
        for t, copies in ((0, 1), (1, S - frames + 1)):
            on = host.clone()
            on[t, 2 * stride, 3 * stride] = bad
            dm, zr = tracker.window_depth(on.to(DEV), S, stride, 0.5, 20.0, W // stride)
            want, zr_want = U.window_depth(on, S, stride, 0.5, 20.0, W // stride, False)
            assert same_values(dm.cpu(), want) and same_values(zr.cpu(), pair(*zr_want)), (bad, t)
            hit = ~torch.isfinite(dm)
            assert int(hit.sum()) == copies and bool(hit[t:t + copies if t else 1, 2, 3].all()), (bad, t)
            assert bool(torch.isnan(zr).all()) if bad != bad else float(zr[1]) == INF


def test_window_depth_log_form_clamps(tracker):
    """use_log_depth at d = 1e-3, below it, 0, -0, negative and -inf: log(1e-3) for all of them.  The bound of
    test_log_depth_range_and_window_depth, against the float64 restatement."""
    frames, S, H, W, stride = 3, 4, 23, 37, 2
    g = torch.Generator().manual_seed(40)
    host = torch.rand(frames, H, W, generator=g) * 19.5 + 0.5
    clamped = [1e-3, 9.99e-4, 1e-30, 1e-40, 0.0, -0.0, -3.0, -INF]
    for k, v in enumerate(clamped):
        host[k % frames, 2 * (k + 1), 4 * k] = v
    d_near, d_far = U.depth_range(host, True)                    # float32 values, as the front end reads them back
    assert abs(d_near - np.log(1e-3)) < 1e-6
    Dz = W // stride
    dm, zr = tracker.window_depth(host.to(DEV), S, stride, d_near, d_far, Dz, True)
    want, __ = U.window_depth(host.double(), S, stride, d_near, d_far, Dz, True)
    bound = 2 * 4.8e-7 * Dz / (d_far - d_near) + 1.5 * float(np.spacing(np.float32(want.abs().max())))
    err = float((dm.cpu().double() - want).abs().max())
    print(f"log clamp: max |window_depth - restatement64| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    at = [float(dm[k % frames, k + 1, 2 * k]) for k in range(len(clamped))]
    assert len(set(at)) == 1 and at[0] == float(dm.min()) == float(zr[0]) and abs(at[0]) <= bound       # all of them the clamp's value
    assert torch.equal(zr, torch.stack([dm.min(), dm.max()])) and torch.equal(dm[3], dm[2])


# ------------------------------------------------------------------------------- 3. embed_conv: one-hot weights
def conv_with(weight, bias):
    conv = torch.nn.Conv2d(U.C + U.EMB, U.C, 3, padding=1)
    conv.weight.data.copy_(weight)
    conv.bias.data.copy_(bias)
    return conv.to(DEV).requires_grad_(False)


def depth_maps(S, h, w, g):
    """Random z with the window's extremes in the first frame's corners, so that |pz| = 1 there."""
    dm = torch.rand(S, h, w, generator=g) * 15 + 1
    dm[:, 0, 0], dm[:, -1, -1] = 0.5, 17.0
    return dm, pair(dm.min(), dm.max())


@pytest.mark.parametrize("h,w", [(9, 17), (16, 33)])
def test_one_hot_weights_pin_the_operand_layout(tracker, h, w):
    """14 convolutions whose 1792 output channels each pick ONE (input channel, tap): together every one of the 191 x 9
    pairs.  out = fl(in[f, c, y + ky - 1, x + kx - 1] + bias[o]) exactly, for the encoder's channels and the normalised
    (x, y, z); within the sine's allowance for the 60 sine and cosine channels, whose arguments reach 1024 rad in the
    corners.  F = 2 frames from frame0 = 1 of S = 3; 2 x 2 (3 x 2) tiles, ragged both ways (the bottom and the right)."""
    S, frame0, F = 3, 1, 2
    g = torch.Generator().manual_seed(1000 * h + w)
    fnet = torch.randn(F, U.C, h, w, generator=g)
    assert float(fnet.abs().min()) > 1e-30                        # no subnormals (and no zeros)
    dm, zr = depth_maps(S, h, w, g)
    p = U.embedding(dm, zr)[frame0:frame0 + F, :3]               # float32 on the CPU: every operation rounded, the division true
    assert float(p.abs().max()) == 1.0 and bool((p[:, :, 0, 0] == -1).all()) and bool((p[:, :, -1, -1] == 1).all())
    exact = torch.cat([fnet, p], 1)                              # input channels 0 .. 130
    freqs = torch.tensor(U.FREQS, dtype=torch.float32)
    arg = (p[:, None] * freqs[None, :, None, None, None])        # ONE float32 multiply: [F, 10, 3, h, w]
    assert float(arg.abs().max()) == 1024.0
    trig = torch.cat([torch.sin(arg.double()), torch.cos(arg.double())], 2).reshape(F, 60, h, w)       # channels 131 .. 190, float64
    taps = U.one_hot_taps()
    fnet_d, dm_d, zr_d = fnet.to(DEV), dm.to(DEV), zr.to(DEV)
    worst, least_bound, seen = 0.0, INF, torch.zeros(U.C + U.EMB, 3, 3, dtype=torch.bool)
    for k in range(U.ONE_HOT_CONVS):
        bias = (torch.rand(U.C, generator=g) + 0.25) * (1 - 2 * (torch.rand(U.C, generator=g) < 0.5).float())
        got = tracker.embed_conv(fnet_d, dm_d, zr_d, frame0, conv_with(U.one_hot_weight(taps[k]), bias), U.FREQS).cpu()
        is_exact = taps[k][:, 0] < U.C + 3
        want = U.one_hot_select(exact, taps[k][is_exact]) + bias[is_exact][None, :, None, None]
        bad = (got[:, is_exact] != want).flatten(2).any(2).any(0)
        assert not bool(bad.any()), (k, "output channels", torch.nonzero(is_exact)[bad].flatten().tolist(), "taps", taps[k][is_exact][bad].tolist())
        t = taps[k][~is_exact].clone()
        t[:, 0] -= U.C + 3
        want64 = U.one_hot_select(trig, t) + bias[~is_exact].double()[None, :, None, None]
        bound = 4 * UNIT + 0.5 * torch.from_numpy(np.spacing((want64.abs() + 4 * UNIT).numpy().astype(np.float32))).double()
        err = (got[:, ~is_exact].double() - want64).abs()
        worst, least_bound = max(worst, float(err.max())), min(least_bound, float(bound.min()))
        assert bool((err <= bound).all()), (k, float((err / bound).max()))
        seen[taps[k][:, 0], taps[k][:, 1], taps[k][:, 2]] = True
    print(f"one-hot {h} x {w}: max |sine, cosine channel - float64 at the float32 argument| {worst:.3e}, bound {least_bound:.3e} at the least")
    assert bool(seen.all())


# -------------------------------------------------------------------- 4. embed_conv: shapes round the tile, frames, strides
TILE_SHAPES = [(2, 2), (2, 17), (9, 2), (8, 16), (9, 16), (8, 17), (7, 15), (17, 33)]


def raw_embed_conv(tracker, fnet, dm, zr, frame0, F, conv, out):
    wp, bias = tracker.packed_conv(conv)
    h, w = dm.shape[1:]
    return _lib.lib().bt_embed_conv(fnet.data_ptr(), *fnet.stride(), dm.data_ptr(), zr.data_ptr(), wp.data_ptr(), bias.data_ptr(),
                                    tracker.freq_table(U.FREQS, fnet.device).data_ptr(), dm.shape[0], frame0, F, h, w, U.C, out.data_ptr(), stream())


@pytest.mark.parametrize("h,w", TILE_SHAPES)
def test_embed_conv_shapes_round_the_tile(tracker, h, w):
    """Random weights, S = 4, F in {1, 3} at frame0 in {0, S - F}: the 2 x convention pooled over the four calls, against
    the float32 and float64 restatements on the CPU.  Each frame alone equals the same frame of the whole window bit for
    bit; channels_last, every other column of a wider buffer (sx = 2) and one frame expanded to F (sf = 0) equal the
    contiguous call bit for bit; F = 0 is an empty result and, through the raw entry point, BT_OK with nothing written."""
    S = 4
    g = torch.Generator().manual_seed(100 * h + w)
    conv, conv_cpu = conv_of("B"), conv_of("B", "cpu")
    fnet = torch.randn(S, U.C, h, w, generator=g)
    dm, zr = depth_maps(S, h, w, g)
    w32, b32 = conv_cpu.weight, conv_cpu.bias
    want32 = U.embed_conv(fnet, dm, zr, 0, w32, b32)
    want64 = U.embed_conv(fnet.double(), dm.double(), zr.double(), 0, w32.double(), b32.double())
    fnet_d, dm_d, zr_d = fnet.to(DEV), dm.to(DEV), zr.to(DEV)
    pool = Pool(f"embed_conv {h} x {w}")
    for F in (1, 3):
        for frame0 in (0, S - F):
            fr = slice(frame0, frame0 + F)
            got = tracker.embed_conv(fnet_d[fr], dm_d, zr_d, frame0, conv, U.FREQS)
            assert got.shape == (F, U.C, h, w) and got.is_contiguous()
            pool.feed("all channels", got.cpu(), want32[fr], want64[fr])
    pool.check()

    full = tracker.embed_conv(fnet_d, dm_d, zr_d, 0, conv, U.FREQS)
    for f in range(S):
        assert torch.equal(tracker.embed_conv(fnet_d[f:f + 1], dm_d, zr_d, f, conv, U.FREQS)[0], full[f]), f
    wide = torch.full((S, U.C, h, 2 * w + 1), NAN, device=DEV)
    wide[..., 1::2] = fnet_d
    views = {"channels_last": fnet_d.to(memory_format=torch.channels_last), "sx = 2": wide[..., 1::2]}
    assert views["channels_last"].stride(1) == 1 and views["sx = 2"].stride(3) == 2
    for name, v in views.items():
        assert torch.equal(tracker.embed_conv(v, dm_d, zr_d, 0, conv, U.FREQS), full), name
    same = fnet_d[1:2].expand(3, U.C, h, w)
    assert same.stride(0) == 0
    got = tracker.embed_conv(same, dm_d, zr_d, 1, conv, U.FREQS)
    for f in range(3):
        assert torch.equal(got[f], tracker.embed_conv(fnet_d[1:2], dm_d, zr_d, 1 + f, conv, U.FREQS)[0]), f

    for frame0 in (0, 2, S):
        empty = tracker.embed_conv(fnet_d[:0], dm_d, zr_d, frame0, conv, U.FREQS)
        assert empty.shape == (0, U.C, h, w) and empty.dtype == torch.float32
        buf = torch.full((U.C * h * w,), SENTINEL, device=DEV)
        assert raw_embed_conv(tracker, fnet_d, dm_d, zr_d, frame0, 0, conv, buf) == _lib.BT_OK
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())


# ----------------------------------------------------------------------------------------- 5. reach of a non-finite value
REACH_AT = [(0, 0), (7, 15), (8, 16), (16, 32)]                  # a corner, either side of a tile border both ways, the last pixel


def test_reach_of_a_non_finite_value_in_embed_conv(tracker):
    """17 x 33 maps (3 x 3 tiles), F = 2 from frame0 = 1 of S = 4.  One NaN in fnet[f, c, y, x], or one NaN or +inf in
    dmaps[frame0 + f, y, x] (sin(inf) is NaN) with the clean maps' finite zrange: NaN at frame f, all 128 channels, rows
    y - 1 .. y + 1 and columns x - 1 .. x + 1 clipped to the map; every other value has the clean call's bits.  A NaN in a
    frame of dmaps outside frame0 .. frame0 + F changes nothing."""
    S, frame0, F, h, w = 4, 1, 2, 17, 33
    g = torch.Generator().manual_seed(51)
    conv = conv_of("A")
    assert int((conv.weight == 0).sum()) == 0
    fnet = torch.randn(F, U.C, h, w, generator=g).to(DEV)
    dm, zr = depth_maps(S, h, w, g)
    dm, zr = dm.to(DEV), zr.to(DEV)
    clean = tracker.embed_conv(fnet, dm, zr, frame0, conv, U.FREQS)
    assert bool(torch.isfinite(clean).all())

    def only(got, f, y, x, what):
        m = torch.zeros(F, U.C, h, w, dtype=torch.bool, device=DEV)
        m[f, :, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
        assert bool(torch.isnan(got[m]).all()), what
        assert torch.equal(got[~m], clean[~m]), what

    for i, (y, x) in enumerate(REACH_AT):
        f = i % F
        for c in (0, 127):
            bad = fnet.clone()
            bad[f, c, y, x] = NAN
            only(tracker.embed_conv(bad, dm, zr, frame0, conv, U.FREQS), f, y, x, ("fnet", c, y, x))
        for v in (NAN, INF):
            bad = dm.clone()
            bad[frame0 + f, y, x] = v
            only(tracker.embed_conv(fnet, bad, zr, frame0, conv, U.FREQS), f, y, x, ("dmaps", v, y, x))
        for t in (0, 3):
            bad = dm.clone()
            bad[t, y, x] = NAN
            assert torch.equal(tracker.embed_conv(fnet, bad, zr, frame0, conv, U.FREQS), clean), ("dmaps, another frame", t, y, x)


# ------------------------------------------------------------------------------------------------------- 6. feat_sample
def far_queries(S, h, w):
    """Every pair of the edge coordinates, the frames cycling through every clamp: (frames int32 [n], xy [n, 2])."""
    def axis(hi):
        return [-0.0, 0.0, float(hi), hi + 0.5, -0.5, 3e9, -3e9, F32_MAX, -F32_MAX, INF, -INF, NAN, 0.25, hi - 0.25]
    frames = [I32_MIN, -1, 0, S - 1, S, I32_MAX]
    xy = torch.tensor([(x, y) for x in axis(w - 1) for y in axis(h - 1)], dtype=torch.float32)
    fr = torch.tensor([frames[(k + k // len(frames)) % len(frames)] for k in range(xy.shape[0])], dtype=torch.int32)
    return fr, xy


@pytest.mark.parametrize("S,h,w", [(1, 1, 1), (3, 1, 1), (3, 1, 9), (1, 9, 1), (3, 9, 1), (2, 5, 7)])
def test_feat_sample_on_thin_maps_at_far_coordinates(tracker, S, h, w):
    """1 x 1, 1 x 9 and 9 x 1 maps, S = 1, frames from INT32_MIN to INT32_MAX, coordinates -0, the last row and column
    exactly, half a pixel outside, +-3e9 (beyond int32: floor_int32's INT_MIN rule), +-FLT_MAX, +-inf and NaN, row strides
    of xy of 2, 3 and 7, and n = 1: the restatement's bits on the CPU, NaN where it has NaN."""
    g = torch.Generator().manual_seed(60 + 10 * h + w)
    fm = torch.randn(S, U.C, h, w, generator=g)
    fm_d = fm.to(DEV)
    fr, xy = far_queries(S, h, w)
    want = U.sample_features(fm, fr, xy)
    assert bool(torch.isnan(want).any()) and bool(torch.isfinite(want).any())
    for frames in (I32_MIN, I32_MAX):                            # the reference clamps, whatever the kernel does
        assert torch.equal(U.sample_features(fm, torch.tensor([frames]), xy[:1]), fm[0 if frames < 0 else S - 1, :, 0, 0][None])
    for row in (2, 3, 7):
        buf = torch.full((xy.shape[0], row), NAN)
        buf[:, :2] = xy
        got = tracker.sample_features(fm_d, fr.to(DEV), buf.to(DEV)[:, :row if row < 7 else 4])
        assert same_values(got.cpu(), want), row
    for k in (0, 5, xy.shape[0] - 1):
        got = tracker.sample_features(fm_d, fr[k:k + 1].to(DEV), xy[k:k + 1].to(DEV))
        assert got.shape == (1, U.C) and same_values(got.cpu(), want[k:k + 1]), k


def test_feat_sample_past_the_grid_cap():
    """n = 2^20 + 5 queries on a 2 x 128 x 4 x 4 map: the block loop takes a second trip for five of them.  Queries k and
    k - 2^20 are the same, so their rows are; no row keeps the sentinel; 4096 drawn rows equal the CPU restatement."""
    if torch.cuda.mem_get_info()[0] < 2 << 30:
        pytest.skip("less than 2 GB of device memory free: the output alone is 512 MB")
    S, h, w, cap = 2, 4, 4, 1 << 20
    n = cap + 5
    g = torch.Generator().manual_seed(70)
    fm = torch.randn(S, U.C, h, w, generator=g)
    gd = torch.Generator(device=DEV).manual_seed(71)
    xy = torch.rand(n, 2, device=DEV, generator=gd) * torch.tensor([w + 2.0, h + 2.0], device=DEV) - 1.5
    fr = torch.randint(-1, S + 1, (n,), device=DEV, generator=gd, dtype=torch.int32)
    xy[cap:], fr[cap:] = xy[:5], fr[:5]
    out = torch.full((n, U.C), SENTINEL, device=DEV)
    fm_d = fm.to(DEV)
    rc = _lib.lib().bt_feat_sample(fm_d.data_ptr(), S, U.C, h, w, fr.data_ptr(), xy.data_ptr(), 2, n, out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == _lib.BT_OK
    assert torch.equal(out[cap:], out[:5])
    assert not bool((out == SENTINEL).any())
    pick = torch.cat([torch.randint(0, n, (4086,), generator=g), torch.arange(5), torch.arange(cap, n)])
    want = U.sample_features(fm, fr.cpu()[pick], xy.cpu()[pick])
    assert torch.equal(out[pick.to(DEV)].cpu(), want)


# --------------------------------------------------------------------------------- 7. guard rows through the raw entry points
def test_guard_rows_through_the_raw_entry_points(tracker):
    """Every input between 64 NaN elements, every output inside a buffer of sentinels, the workspace followed by 64
    sentinel bytes; 9 x 17 maps from a 39 x 69 image, F = 2 as the slice frame0 = 1 of S = 4, 3 frames of depth, n = 37.
    The results equal the front end's on plain tensors, nothing non-finite is read, no sentinel is written."""
    L = _lib.lib()
    S, frames, frame0, F, H, W, stride, n = 4, 3, 1, 2, 39, 69, 4, 37
    h, w = H // stride, W // stride
    assert (h, w) == (9, 17)
    g = torch.Generator().manual_seed(80)
    depth = (torch.rand(frames, H, W, generator=g) * 19.5 + 0.5).to(DEV)
    depth[0, 0, 0] = 0.0
    conv = conv_of("A")
    ws = Workspace()

    want = tracker.depth_range(depth)
    d_near, d_far = want.tolist()
    dbuf, d = guarded(depth, NAN)
    d = d.view_as(depth)
    obuf, out = guarded(torch.full((2,), SENTINEL), SENTINEL)
    assert L.bt_depth_range(d.data_ptr(), *d.shape, *d.stride(), 0, ws.buf.data_ptr(), out.data_ptr(), stream()) == _lib.BT_OK
    ws.settle()
    assert torch.equal(out, want) and untouched(obuf)

    dm_want, zr_want = tracker.window_depth(depth, S, stride, d_near, d_far, w)
    mbuf, dm = guarded(torch.full((S, h, w), SENTINEL), SENTINEL)
    zbuf, zr = guarded(torch.full((2,), SENTINEL), SENTINEL)
    rc = L.bt_window_depth(d.data_ptr(), frames, S, H, W, *d.stride(), stride, d_near, d_far - d_near, float(w), 0, ws.buf.data_ptr(),
                           dm.data_ptr(), zr.data_ptr(), stream())
    assert rc == _lib.BT_OK
    ws.settle()
    assert torch.equal(dm.view_as(dm_want), dm_want) and torch.equal(zr, zr_want) and untouched(mbuf) and untouched(zbuf)
    assert bool(torch.isfinite(dm_want).all()) and bool(torch.isfinite(zr_want).all())

    fnet = torch.randn(F, U.C, h, w, generator=g).to(DEV)
    fm_want = tracker.embed_conv(fnet, dm_want, zr_want, frame0, conv, U.FREQS)
    wp, bias = tracker.packed_conv(conv)
    nan = [guarded(t, NAN) for t in (fnet, dm_want, zr_want, wp, bias, tracker.freq_table(U.FREQS, DEV))]
    assert nan[3][1].data_ptr() % 16 == 0
    obuf, out = guarded(torch.full_like(fm_want, SENTINEL), SENTINEL)
    rc = L.bt_embed_conv(nan[0][1].data_ptr(), *fnet.stride(), *(t[1].data_ptr() for t in nan[1:]), S, frame0, F, h, w, U.C, out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == _lib.BT_OK and torch.equal(out.view_as(fm_want), fm_want) and untouched(obuf) and bool(torch.isfinite(fm_want).all())

    fmaps = torch.randn(S, U.C, h, w, generator=g).to(DEV)
    fr = torch.randint(-1, S + 1, (n,), generator=g, dtype=torch.int32).to(DEV)
    xy = (torch.rand(n, 3, generator=g) * torch.tensor([w + 4.0, h + 4.0, 1.0]) - 2.0).to(DEV)
    fs_want = tracker.sample_features(fmaps, fr, xy)
    assert bool(torch.isfinite(fs_want).all())
    fbuf, fm = guarded(fmaps, NAN)
    xbuf, x = guarded(xy, NAN)
    ibuf = torch.full((n + 2 * GUARD,), 1 << 30, dtype=torch.int32, device=DEV)
    ibuf[GUARD:GUARD + n] = fr
    obuf, out = guarded(torch.full_like(fs_want, SENTINEL), SENTINEL)
    rc = L.bt_feat_sample(fm.data_ptr(), S, U.C, h, w, ibuf[GUARD:].data_ptr(), x.data_ptr(), 3, n, out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == _lib.BT_OK and torch.equal(out.view_as(fs_want), fs_want) and untouched(obuf)
