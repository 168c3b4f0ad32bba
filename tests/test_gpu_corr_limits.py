"""The fused correlation lookup at its limits (include/batrack_corr.h, batrack_amd/csrc/corr_lookup.hip): the generic
kernel at the largest C, r and L and at the smallest, maps smaller than the window and levels pooled down to 1 x 1, the
tuned shape on such maps, the pyramid buffer itself, coordinates a network can put out (far away, non-finite), every
coordinate layout through both bindings, and the refusals on the device.

Reference and gate.  The reference is tests/corr_util.np_corr_lookup in float64 on the same float32-valued inputs (the CPU
suite ties it to the reference's fixture and, on the edge inputs used here, to the volume formulation).  The gate is
measured in every case from that restatement alone: e32 = max |np_corr_lookup(float32) - np_corr_lookup(float64)|; the
kernel may be 2 x e32 away (the project's margin for a fused kernel that sums in another order, test_gpu_world_tracks.py),
with a floor of one float32 unit of the largest |ref| for the cases whose e32 is 0.  No gate is taken from the kernel.
The pyramid is held to bit equality: the pool kernel computes (((a + b) + c) + d) * 0.25 in float32 and nothing else — no
product feeds an add, so there is nothing to contract — and np_pyramid(float32) uses the same order.
Every case prints its error beside its gate."""
import os

import numpy as np
import pytest
import torch

import corr_util
from batrack_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
FAR = 2                                                              # make_inputs' query at (-40, -40)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device=DEV)


def fused(fmaps, targets, coords, L, r):
    """CorrBlock on tensors [B,S,...] (numpy arrays [S,...] get the batch dimension here)."""
    from batrack_amd.frontend.corr import CorrBlock
    fmaps, targets, coords = (dev(a)[None] if isinstance(a, np.ndarray) else a for a in (fmaps, targets, coords))
    blk = CorrBlock(fmaps, num_levels=L, radius=r)
    blk.corr(targets)
    return blk.sample(coords)


def reference(fmaps, targets, coords, L, r):
    """(float64 restatement, gate): frame by frame, so that the numpy gather stays small."""
    ref, r32 = (np.concatenate([corr_util.np_corr_lookup(fmaps[s:s + 1], targets[s:s + 1], coords[s:s + 1], L, r, dt)
                                for s in range(len(fmaps))]) for dt in (np.float64, np.float32))
    e32 = float(np.abs(r32.astype(np.float64) - ref).max())
    return ref, max(2.0 * e32, float(np.spacing(np.float32(np.abs(ref).max())))), e32


def check(desc, fmaps, targets, coords, L, r):
    """One lookup against the float64 restatement under the restatement's own float32 error; returns the kernel's output."""
    S, N = coords.shape[:2]
    d = 2 * r + 1
    ref, gate, e32 = reference(fmaps, targets, coords, L, r)
    out = fused(fmaps, targets, coords, L, r)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (1, S, N, L * d * d)
    got = out[0].cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref).max())
    print(f"{desc}: max |kernel - ref64| {err:.3e}, gate {gate:.3e} (e32 {e32:.3e}, max |ref| {np.abs(ref).max():.3g})")
    assert 0 < gate < 1e-3, gate
    assert np.isfinite(got).all()
    assert err <= gate, (desc, err, gate)
    assert not got[ref == 0].any(), desc                             # wholly outside: exactly 0, not small
    assert torch.equal(out, fused(fmaps, targets, coords, L, r))     # bit-stable from call to call
    return got, ref


def lookup_into_padded_buffer(fmaps, targets, coords, L, r, pad):
    """bt_corr_lookup through the C ABI with `out` at the head of a sentinel-filled buffer `pad` floats longer: returns
    (out [S,N,L*d*d], the padding) as numpy.  A wave past the last work item that wrote would write into the padding."""
    from batrack_amd.frontend.corr import CorrBlock
    (S, N), (C, H, W) = coords.shape[:2], fmaps.shape[1:]
    n = S * N * L * (2 * r + 1) ** 2
    blk = CorrBlock(dev(fmaps)[None], num_levels=L, radius=r)
    buf = torch.full((n + pad,), SENTINEL, device=DEV)
    tg, co = dev(targets).contiguous(), dev(coords).contiguous()
    rc = _lib.lib().bt_corr_lookup(blk.pyramid.data_ptr(), S, C, H, W, L, r, tg.data_ptr(), co.data_ptr(), 2, N, buf.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.BT_OK, rc
    return buf[:n].view(S, N, -1).cpu().numpy(), buf[n:].cpu().numpy()


GENERIC = [(512, 7, 1, 20, 24, 2, 8),       # the second trip of the target staging (C/4 = 128) and four of the output loop (225 > 64)
           (4, 0, 1, 9, 7, 1, 1),           # one work item; one float4 a row, 15 of 16 lanes idle; r = 0
           (36, 1, 2, 10, 13, 3, 5),        # 30 items: the last block has two idle waves; 9 float4 a row; a partial channel tile
           (64, 7, 3, 4, 4, 1, 7),          # the map inside the window, the last level 1 x 1
           (8, 2, 1, 1, 37, 2, 6),          # one row
           (8, 2, 1, 37, 1, 2, 6),          # one column
           (512, 7, 8, 128, 130, 1, 4)]     # every limit at once; 130 -> 65 -> 32: 1 x 1 after odd floors


@pytest.mark.parametrize("C,r,L,H,W,S,N", GENERIC)
def test_generic_kernel_at_its_limits(C, r, L, H, W, S, N):
    assert (min(H, W) >> (L - 1)) >= 1
    fmaps, targets, coords = corr_util.limit_inputs(1000 + C + r + L + H, S, C, H, W, max(N, 4))
    assert (coords[:, 0] == 0).all() and (coords[:, 1] == (W - 1, H - 1)).all() and (coords[:, FAR] == -40).all()
    assert (coords[:, 3] * 4 == np.round(coords[:, 3] * 4)).all()
    d = 2 * r + 1
    if N >= 4:
        got, ref = check(f"C {C} r {r} L {L} {H}x{W} S {S} N {N}", fmaps, targets, coords, L, r)
        assert not ref[:, FAR, :d * d].any() and not got[:, FAR, :d * d].any()          # level 0 of the far query: exactly 0
        raw, padding = lookup_into_padded_buffer(fmaps, targets, coords, L, r, 4 * d * d)
        assert np.array_equal(raw.astype(np.float64), got) and (padding == SENTINEL).all()   # nothing past the last work item
    else:                                    # N = 1: the four special queries one at a time, each a single work item
        assert S * N * L == 1
        for q in range(4):
            got, ref = check(f"C {C} r {r} L {L} {H}x{W} S {S} N {N}, special query {q}", fmaps, targets[:, q:q + 1], coords[:, q:q + 1], L, r)
            assert (q == FAR) == (not ref.any())
            assert (q == FAR) == (not got.any())
            raw, padding = lookup_into_padded_buffer(fmaps, targets[:, q:q + 1], coords[:, q:q + 1], L, r, 4 * d * d)
            assert np.array_equal(raw.astype(np.float64), got) and (padding == SENTINEL).all()   # three idle waves wrote nothing


@pytest.mark.parametrize("L,H,W", [(8, 128, 130), (3, 4, 5)])
def test_tuned_shape_at_the_limits(L, H, W):
    """C = 128, r = 3 through both lane layouts and the generic kernel: the deepest pyramid (1 x 1 after odd floors) and a map
    inside the window (4 x 5 -> 2 x 2 -> 1 x 1); 9 queries, so that the last block of the L = 3 run has an idle wave."""
    C, r, S, N = 128, 3, 1, 9
    fmaps, targets, coords = corr_util.limit_inputs(2000 + L, S, C, H, W, N)
    prev = _lib.lib().bt_config_corr_lookup_layout(-1)
    try:
        for lay in (0, 1, 2):
            _lib.lib().bt_config_corr_lookup_layout(lay)
            assert _lib.lib().bt_config_corr_lookup_layout(-1) == lay
            got, ref = check(f"C {C} r {r} L {L} {H}x{W} layout {lay}", fmaps, targets, coords, L, r)
            assert not ref[:, FAR, :49].any() and not got[:, FAR, :49].any()
    finally:
        _lib.lib().bt_config_corr_lookup_layout(prev)


def packed_pyramid(fmaps32, L):
    """np_pyramid(float32) channels-last, packed at the header's offsets: level l is [S', H_l, W_l, C]."""
    return np.concatenate([f.transpose(0, 2, 3, 1).ravel() for f in corr_util.np_pyramid(fmaps32, L)])


@pytest.mark.parametrize("S,C,H,W,L", [(2, 36, 45, 61, 3),        # a partial channel tile (36 = 32 + 4), a partial pixel tile, odd floors
                                       (1, 128, 1, 37, 1),        # one row, one level
                                       (24, 128, 96, 128, 4)])    # 18,432 level-0 tiles and 2,359,296 float4 at level 1: past one pass of both grids
def test_pyramid_bit_for_bit(S, C, H, W, L):
    from batrack_amd.frontend.corr import CorrBlock
    rng = np.random.default_rng(3000 + S + C)
    fmaps = rng.standard_normal((S, C, H, W), dtype=np.float32)
    want = packed_pyramid(fmaps, L)
    sizes = corr_util.level_sizes(H, W, L)
    assert want.size == C * S * sum(h * w for h, w in sizes) == _lib.lib().bt_corr_pyramid_bytes(S, C, H, W, L) // 4
    if S == 24:
        assert S * (C // 32) * (H * W // 64) == 18432 > 8192 and S * sizes[1][0] * sizes[1][1] * (C // 4) == 2359296 > 8192 * 256
    blk = CorrBlock(dev(fmaps)[None], num_levels=L, radius=3)
    got = blk.pyramid.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    off = 0
    for l, (h, w) in enumerate(sizes):
        n = S * h * w * C
        differ = int((got[off:off + n].view(np.int32) != want[off:off + n].view(np.int32)).sum())
        print(f"pyramid S' {S} C {C} {H}x{W} level {l} ({h}x{w}) at float offset {off}: {differ} of {n} elements differ (gate: 0)")
        assert differ == 0, (l, differ)
        off += n
    if S == 24:                              # and a lookup of 64 queries a frame through the large pyramid
        N = 64
        g = np.random.default_rng(3001)
        targets = g.standard_normal((S, N, C), dtype=np.float32).astype(np.float64)
        coords = corr_util.make_inputs(3002, S, 4, H, W, N)[2][0, ..., :2]
        blk.corr(dev(targets)[None])
        out = blk.sample(dev(coords)[None])[0].cpu().numpy().astype(np.float64)
        ref, gate, e32 = reference(fmaps, targets, coords, L, 3)
        err = float(np.abs(out - ref).max())
        print(f"lookup through it, S' {S} N {N}: max |kernel - ref64| {err:.3e}, gate {gate:.3e} (e32 {e32:.3e})")
        assert 0 < gate < 1e-3 and err <= gate, (err, gate)
        assert not out[:, FAR].any() and not ref[:, FAR].any()


@pytest.mark.parametrize("C,r,L,H,W,layout", [(128, 3, 4, 48, 64, 0), (128, 3, 4, 48, 64, 1), (64, 4, 3, 45, 61, 0)])
def test_far_and_non_finite_coordinates(C, r, L, H, W, layout):
    """corr_util.edge_queries planted among ordinary queries.  Expected: the volume formulation in float64 on the CPU,
    computed here — all-NaN for a query with a non-finite coordinate, exactly 0 for a far one, the restatement elsewhere —
    which is the header: a tap outside the map contributes exactly 0 and a non-finite fraction propagates."""
    S, N, d = 2, 64, 2 * r + 1
    fmaps, targets, coords, kinds, calm = corr_util.planted_inputs(4000 + C, S, C, H, W, N, r)
    nonfinite, planted = kinds == "nonfinite", kinds != ""
    assert np.array_equal(nonfinite, ~np.isfinite(coords).all((0, 2))) and nonfinite.any()
    with np.errstate(all="ignore"):
        vol = corr_util.volume_lookup_cpu64(fmaps, targets, coords, L, r)
    finite_coords = np.where(nonfinite[None, :, None], calm, coords)
    ref, gate, e32 = reference(fmaps, targets, finite_coords, L, r)
    assert np.isnan(vol[:, nonfinite]).all() and np.isfinite(vol[:, ~nonfinite]).all()   # the expected non-finite pattern
    assert np.abs(vol[:, ~nonfinite] - ref[:, ~nonfinite]).max() <= 1e-12                # the two formulations, finite queries
    assert not ref[:, kinds == "far"].any() and not ref[:, kinds == "outside", :d * d].any() and not ref[:, FAR].any()
    prev = _lib.lib().bt_config_corr_lookup_layout(-1)
    try:
        _lib.lib().bt_config_corr_lookup_layout(layout)
        out = fused(fmaps, targets, coords, L, r)
        out_calm = fused(fmaps, targets, calm, L, r)
    finally:
        _lib.lib().bt_config_corr_lookup_layout(prev)
    got = out[0].cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        err = float(np.abs(got - ref)[:, ~nonfinite].max())
    nan_kernel, inf_kernel = np.isnan(got), np.isinf(got)
    print(f"C {C} r {r} L {L} {H}x{W} layout {layout}: finite queries max |kernel - ref64| {err:.3e}, gate {gate:.3e} (e32 {e32:.3e}); "
          f"queries with a non-finite coordinate: {int(nan_kernel[:, nonfinite].sum())} of {nan_kernel[:, nonfinite].size} outputs NaN, "
          f"{int(inf_kernel.sum())} inf; NaN elsewhere: {int(nan_kernel[:, ~nonfinite].sum())}")
    assert np.array_equal(~np.isfinite(got), np.isnan(vol))          # the non-finite pattern, exactly
    assert nan_kernel[:, nonfinite].all() and not nan_kernel[:, ~nonfinite].any() and not inf_kernel.any()
    assert not got[:, kinds == "far"].any()                          # +-3e9, +-(1e6 +- 0.5), 2^24 + 1: exactly 0
    assert not got[:, kinds == "outside", :d * d].any()              # W + r, -r - 1: the first wholly outside, level 0
    assert not got[:, ~nonfinite][ref[:, ~nonfinite] == 0].any()
    assert 0 < gate < 1e-3 and err <= gate, (err, gate)
    others = torch.as_tensor(~planted, device=DEV)
    assert torch.equal(out[0][:, others], out_calm[0][:, others])    # the neighbours of a planted query: bit-equal without it
    assert others.sum() >= corr_util.N_SPECIAL


# ---------------------------------------------------------------------------------- both bindings, every coordinate layout
def layouts_through(route, monkeypatch, C, r, L, H, W):
    """Every coordinate layout through one binding ('ops': torch.ops.batrack_hip as loaded; 'ctypes': the C ABI from Python,
    taken when torch_ops() returns None), each torch.equal to the same binding's packed call.  Returns name -> output."""
    from batrack_amd.frontend.corr import CorrBlock
    if route == "ops":
        if os.environ.get("BT_LIB_PATH") or not os.path.exists(_lib.TORCH_LIB_PATH):
            pytest.skip("libbatrack_torch.so is not built for this copy of the C library: only the ctypes route can run")
        assert _lib.torch_ops(strict=True) is not None               # a library that is there and does not load is a failure
    else:
        monkeypatch.setattr(_lib, "torch_ops", lambda strict=False: None)
    B, S, N = 2, 3, 40
    fm, tg, c3 = (dev(a) for a in corr_util.make_inputs(5000 + C, S, C, H, W, N, B=B))
    xy = c3[..., :2].contiguous()
    c4 = torch.full((B, S, N, 4), float("nan"), device=DEV)
    c4[..., 1:3] = xy

    def sample(fmaps, targets, coords):
        blk = CorrBlock(fmaps, num_levels=L, radius=r)
        blk.corr(targets)
        out = blk.sample(coords)
        assert out.shape == (*coords.shape[:3], L * (2 * r + 1) ** 2) and out.is_contiguous() and bool(torch.isfinite(out).all())
        return out

    one = xy[:, :, 7:8]
    views = dict(packed=(fm, tg, xy),
                 view_of_three=(fm, tg, c3[..., :2]),
                 view_of_four=(fm, tg, c4[..., 1:3]),
                 batch_slice=(fm[1:2], tg[1:2], c3[1:2, ..., :2]),
                 query_slice=(fm, tg[:, :, 5:37], c3[:, :, 5:37, :2]),
                 expanded=(fm, tg, one.expand(B, S, N, 2)),
                 frames_transposed=(fm, tg, xy.transpose(1, 2).contiguous().transpose(1, 2)),
                 pairs_transposed=(fm, tg, xy.transpose(2, 3).contiguous().transpose(2, 3)),
                 single=(fm[:1, :1], tg[:1, :1, 3:4], c3[:1, :1, 3:4, :2]),
                 empty=(fm, tg[:, :, :0], c3[:, :, :0, :2]))
    assert views["view_of_three"][2].stride() == (S * N * 3, N * 3, 3, 1) and views["view_of_four"][2].stride(-2) == 4
    assert views["view_of_four"][2].storage_offset() == 1 and views["batch_slice"][2].storage_offset() == S * N * 3
    assert views["query_slice"][2].stride(1) != 32 * 3 and views["expanded"][2].stride(2) == 0
    assert views["frames_transposed"][2].stride() == (S * N * 2, 2, 2 * S, 1) and views["pairs_transposed"][2].stride(-1) == N
    assert views["single"][2].numel() == 2 and views["single"][2].stride(-2) == 3
    outs = {}
    for name, (f, t, c) in views.items():
        outs[name] = sample(f, t, c)
        assert torch.equal(outs[name], sample(f, t, c.contiguous())), (route, name)       # the binding's own packed call
    assert outs["empty"].shape == (B, S, 0, L * (2 * r + 1) ** 2) and outs["empty"].numel() == 0
    assert torch.equal(outs["batch_slice"], outs["packed"][1:2]) and torch.equal(outs["query_slice"], outs["packed"][:, :, 5:37])
    assert torch.equal(outs["single"], outs["packed"][:1, :1, 3:4])
    assert torch.equal(outs["expanded"][:, :, 7], outs["packed"][:, :, 7])
    return outs


SHAPES = [(128, 3, 4, 48, 64), (64, 4, 3, 45, 61)]


@pytest.mark.parametrize("route", ["ops", "ctypes"])
@pytest.mark.parametrize("C,r,L,H,W", SHAPES)
def test_every_coordinate_layout_through_one_binding(route, C, r, L, H, W, monkeypatch):
    outs = layouts_through(route, monkeypatch, C, r, L, H, W)
    print(f"{route}: {len(outs)} layouts equal to the packed call, C {C} r {r}")


@pytest.mark.parametrize("C,r,L,H,W", SHAPES)
def test_the_two_bindings_agree_on_every_layout(C, r, L, H, W, monkeypatch):
    a = layouts_through("ops", monkeypatch, C, r, L, H, W)
    b = layouts_through("ctypes", monkeypatch, C, r, L, H, W)
    assert a.keys() == b.keys() and len(a) == 10
    for name in a:
        assert torch.equal(a[name], b[name]), name


# ---------------------------------------------------------------------------------- refusals on the device
@pytest.mark.parametrize("change,code", [(dict(L=6), "BT_EINVAL"), (dict(r=8), "BT_EUNSUPPORTED"), (dict(C=516), "BT_EUNSUPPORTED")])
def test_refusals_leave_the_outputs_untouched(change, code):
    """Real device buffers, large enough for the refused sizes: whatever is refused writes nothing."""
    a = dict(S=2, C=128, H=16, W=16, L=4, r=3, N=8)
    a.update(change)
    S, C, H, W, L, r, N = (a[k] for k in ("S", "C", "H", "W", "L", "r", "N"))
    L_ = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    new = lambda n: torch.full((n,), SENTINEL, device=DEV)
    fmaps, targets = torch.randn(S, C, H, W, device=DEV), torch.randn(S, N, C, device=DEV)
    coords = torch.rand(S, N, 2, device=DEV) * 15
    pyr, out = new(2 * S * C * H * W), new(S * N * L * (2 * r + 1) ** 2)
    if "r" not in change:
        assert L_.bt_corr_pyramid_bytes(S, C, H, W, L) == 0
        rc = L_.bt_corr_pyramid(fmaps.data_ptr(), S, C, H, W, L, pyr.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == getattr(_lib, code), rc
        assert bool((pyr == SENTINEL).all())
    rc = L_.bt_corr_lookup(pyr.data_ptr(), S, C, H, W, L, r, targets.data_ptr(), coords.data_ptr(), 2, N, out.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == getattr(_lib, code), rc
    assert bool((out == SENTINEL).all()) and bool((pyr == SENTINEL).all())
    # and the same call without the change goes through
    good = fused(torch.randn(1, 2, 128, 16, 16, device=DEV), torch.randn(1, 2, 8, 128, device=DEV), coords[None], 4, 3)
    assert bool(torch.isfinite(good).all()) and good.shape == (1, 2, 8, 4 * 49)
