"""GPU half of the fused correlation lookup (batrack_amd/csrc/corr_lookup.hip): the kernels against the reference's
fixture under the reference's own float32 error, and at the tracker's real shapes against the volume formulation of
tests/corr_util.py run in float64 on the same GPU, under that formulation's own float32 error computed here — no gate
is derived from the kernel under test."""
import types

import numpy as np
import pytest
import torch

import corr_util

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = dict(np.load(corr_util.GOLD))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device=DEV)


def fused(fmaps, targets, coords, L, r):
    from batrack_amd.frontend.corr import CorrBlock
    blk = CorrBlock(fmaps, num_levels=L, radius=r)
    blk.corr(targets)
    return blk.sample(coords)


def real_inputs(seed, S, N, C=128, H=96, W=128, B=1):
    """Device tensors of a tracker-sized call; coords3 [B,S,N,3] as the tracker holds them."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    fmaps = torch.randn(B, S, C, H, W, device=DEV, generator=g)
    targets = torch.randn(B, S, N, C, device=DEV, generator=g)
    u = torch.rand(B, S, N, 3, device=DEV, generator=g)
    coords3 = torch.stack([u[..., 0] * (W + 15) - 8, u[..., 1] * (H + 15) - 8, u[..., 2]], -1).contiguous()   # up to 8 px outside
    coords3[..., 0, :2] = -40.0                                      # a window wholly outside in every frame
    return fmaps, targets, coords3


def slice_gate(fmaps, targets, coords, L, r, sl):
    """The volume formulation on the queries `sl`: its float64 run, and the max |float32 run - float64 run| (the gate)."""
    t, c = targets[:, :, sl], coords[:, :, sl]
    v64 = corr_util.volume_lookup(fmaps.double(), t.double(), c.double(), L, r)
    v32 = corr_util.volume_lookup(fmaps, t.contiguous(), c.contiguous(), L, r).double()
    return v64, float((v32 - v64).abs().max())


@pytest.mark.parametrize("c", list(corr_util.CASES))
def test_fixture_cases_within_the_references_float32_error(c):
    fmaps, targets, coords3, spec = corr_util.load_case(c)
    ref, gate = D[f"{c}.ref"].astype(np.float64), float(D[f"gate.{c}"])
    fm, tg, c3 = dev(fmaps)[None], dev(targets)[None], dev(coords3)[None]
    out = fused(fm, tg, c3[..., :2], spec["L"], spec["r"])
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (1,) + ref.shape
    got = out[0].cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"case {c}: max |kernel - ref64| {err:.3e}, gate {gate:.3e}")
    assert err <= gate, (err, gate)
    assert (ref == 0).any() and not got[ref == 0].any()              # windows wholly outside: exactly 0
    again = fused(fm, tg, c3[..., :2], spec["L"], spec["r"])
    assert torch.equal(out, again)                                   # bit-stable from call to call
    packed = fused(fm, tg, c3[..., :2].contiguous(), spec["L"], spec["r"])
    assert torch.equal(out, packed)                                  # the strided view and a two-column tensor


@pytest.mark.parametrize("N", [1536, 2400])
def test_real_shape_against_the_float64_volume(N):
    S, L, r = 12, 4, 3
    fmaps, targets, coords3 = real_inputs(7 + N, S, N)
    coords = coords3[..., :2]
    out = fused(fmaps, targets, coords, L, r)
    assert out.shape == (1, S, N, L * 49)
    sl = slice(N - 128 - 5, N - 5)
    sl0 = slice(0, 128)
    for s_ in (sl0, sl):
        v64, gate = slice_gate(fmaps, targets, coords, L, r, s_)
        err = float((out[:, :, s_].double() - v64).abs().max())
        print(f"N {N} queries {s_.start}:{s_.stop}: max |kernel - volume64| {err:.3e}, gate (volume32 vs volume64) {gate:.3e}")
        assert 0 < gate < 1e-3
        assert err <= gate, (err, gate)
    assert not out[:, :, 0].any()                                    # (-40, -40): exactly 0


def test_nan_in_a_border_row_shows_where_the_volume_shows_it():
    S, N, L, r = 12, 1536, 4, 3
    fmaps, targets, coords3 = real_inputs(3, S, N)
    # queries around the planted row, inside and outside the map, on non-integer positions
    g = torch.Generator(device=DEV).manual_seed(5)
    coords3[:, :, 1:128, 0] = 40.0 + (torch.rand(1, S, 127, device=DEV, generator=g) - 0.5) * 24 + 0.013
    coords3[:, :, 1:128, 1] = (torch.rand(1, S, 127, device=DEV, generator=g) - 0.6) * 20 + 0.017
    fmaps[0, 3, 17, 0, 40] = float("nan")                            # frame 3, the top border row, one channel
    coords = coords3[..., :2]
    out = fused(fmaps, targets, coords, L, r)
    sl = slice(0, 128)
    v64 = corr_util.volume_lookup(fmaps.double(), targets[:, :, sl].double(), coords[:, :, sl].double(), L, r)
    bad, want = ~torch.isfinite(out[:, :, sl]), ~torch.isfinite(v64)
    assert want.any() and want[0, 3].any() and not want[0, :3].any()
    assert torch.equal(bad, want)
    assert not out[:, :, 0].any()                                    # the window wholly outside stays exactly 0
    assert torch.isfinite(out[:, :, 128:]).sum() > 0.99 * out[:, :, 128:].numel()


def test_no_volume_is_allocated():
    from batrack_amd.frontend.corr import CorrBlock
    S, N, L, r = 12, 1536, 4, 3
    fmaps, targets, coords3 = real_inputs(11, S, N)
    blk = CorrBlock(fmaps, num_levels=L, radius=r)
    coords = coords3[..., :2]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    blk.corr(targets)
    out = blk.sample(coords)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    cap = out.numel() * 4 + targets.numel() * 4 + S * N * 2 * 4 + (1 << 20)
    print(f"peak rise {rise} bytes, cap {cap} bytes (the volume would be {4 * S * N * (12288 + 3072 + 768 + 192)})")
    assert rise <= cap, (rise, cap)


def test_batch_of_two_equals_two_blocks():
    S, N, L, r = 3, 40, 4, 3
    fmaps, targets, coords3 = real_inputs(13, S, N, H=48, W=64, B=2)
    both = fused(fmaps, targets, coords3[..., :2], L, r)
    assert both.shape == (2, S, N, L * 49)
    for b in range(2):
        one = fused(fmaps[b:b + 1], targets[b:b + 1], coords3[b:b + 1, ..., :2], L, r)
        assert torch.equal(both[b:b + 1], one)


@pytest.mark.parametrize("C,r,L,H,W", [(64, 4, 3, 45, 61), (256, 2, 2, 40, 56), (128, 3, 4, 96, 128)])
def test_generic_path_against_the_float64_volume(C, r, L, H, W):
    """The last case runs the tuned shape through the generic kernel and both tuned lane layouts: all under the gate."""
    from batrack_amd import _lib
    S, N = 3, 96
    fmaps, targets, coords3 = real_inputs(17 + C, S, N, C=C, H=H, W=W)
    coords = coords3[..., :2]
    v64, gate = slice_gate(fmaps, targets, coords, L, r, slice(0, N))
    layouts = (0, 1, 2) if (C, r) == (128, 3) else (0,)
    prev = _lib.lib().bt_config_corr_lookup_layout(-1)
    try:
        for lay in layouts:
            _lib.lib().bt_config_corr_lookup_layout(lay)
            out = fused(fmaps, targets, coords, L, r)
            err = float((out.double() - v64).abs().max())
            print(f"C {C} r {r} L {L} layout {lay}: max |kernel - volume64| {err:.3e}, gate {gate:.3e}")
            assert out.shape == (1, S, N, L * (2 * r + 1) ** 2)
            assert 0 < gate < 1e-3 and err <= gate, (err, gate)
            assert not out[:, :, 0].any()
    finally:
        _lib.lib().bt_config_corr_lookup_layout(prev)


def test_install_on_a_stand_in_tracker():
    """A module whose loop is the tracker's: one CorrBlock per window, then corr + sample per refinement iteration, six
    times (md_tracker.py forward_iteration: I + static_iters)."""
    from batrack_amd.frontend import corr
    tracker = types.ModuleType("stand_in_tracker")
    tracker.CorrBlock = None

    def forward_iteration(fmaps, targets, coords3, iters=6):
        fcorr_fn = tracker.CorrBlock(fmaps, num_levels=4, radius=3)
        outs = []
        for it in range(iters):
            fcorr_fn.corr(targets)
            outs.append(fcorr_fn.sample((coords3 + 0.37 * it)[..., :2]))
        return outs

    assert corr.install(tracker) is None
    fmaps, targets, coords3 = real_inputs(19, 4, 64, H=48, W=64)
    outs = forward_iteration(fmaps, targets, coords3)
    for it, o in enumerate(outs):
        assert torch.equal(o, fused(fmaps, targets, (coords3 + 0.37 * it)[..., :2], 4, 3))
    assert not torch.equal(outs[0], outs[1])
