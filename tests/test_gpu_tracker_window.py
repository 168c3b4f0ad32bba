"""GPU half of the tracker's window loop (include/batrack_window.h, batrack_amd/frontend/tracker.py) against the reference's
fixture (tests/golden/tracker_window.npz) and the restatement in tests/tracker_window_util.py.  No bound here comes from the
kernels under test: the gates are the reference's own float32-vs-float64 differences, stored in the fixture, or the
restatement's, computed here.  Twice the gate where the kernel and the reference both round on their own: they share the
rounding of the embedding's arguments (up to 1024 rad), and each adds its own rounding of the sum."""
import types

import numpy as np
import pytest
import torch

import tracker_window_util as U

pytestmark = pytest.mark.gpu

D = dict(np.load(U.GOLD))
DEV = "cuda:0"


def gpu(a, dtype=torch.float32):
    return torch.as_tensor(a, dtype=dtype, device=DEV)


def windows(c):
    """(k, ind, prev, n) of the fixture's windows: the start frame and the track counts before and after."""
    spec, out, prev = U.CASES[c], [], 0
    S, first = spec["S"], sorted(spec["first"])
    for ind in range(0, spec["T"] - S // 2, S // 2):
        n = sum(f < ind + S for f in first)
        assert n > 0                                             # every window of the fixture's cases has a query
        out.append((len(out), ind, prev, n))
        prev = n
    return out


def full_fmaps(c, k):
    """The whole window's feature maps of the reference's float32 run, put together as the window loop does."""
    S = U.CASES[c]["S"]
    f = torch.from_numpy(D[f"{c}.0.fmaps"])
    for j in range(1, k + 1):
        f = torch.cat([f[S // 2:], torch.from_numpy(D[f"{c}.{j}.fmaps"])], 0)
    return f


def conv_of(c, device=DEV, dtype=torch.float32):
    return U.StandIn(c, dtype, device, U.embed3d_stand_in()).embedConv


@pytest.fixture(scope="module")
def tracker():
    from batrack_amd.frontend import tracker
    return tracker


@pytest.mark.parametrize("c", list(U.CASES))
def test_depth_range_and_window_depth_are_bit_equal(tracker, c):
    spec = U.CASES[c]
    depth = U.case_tensors(c, device=DEV)["rgbds"][0, :, 3]                  # the strided channel view, read in place
    assert not depth.is_contiguous()
    d_near, d_far = tracker.depth_range(depth).tolist()
    assert (d_near, d_far) == tuple(D[f"{c}.d_range"])
    assert d_near > 0.01                                                     # the masked zeros are not the minimum
    for k, ind, _, _ in windows(c):
        dm, zr = tracker.window_depth(depth[ind:ind + spec["S"]], spec["S"], U.STRIDE, d_near, d_far, spec["W"] // U.STRIDE)
        want = torch.from_numpy(D[f"{c}.{k}.dmaps"])[0, :, 0]
        assert torch.equal(dm.cpu(), want), (c, k)
        assert torch.equal(zr.cpu(), torch.stack([want.min(), want.max()])), (c, k)


def test_log_depth_range_and_window_depth(tracker):
    """use_log_depth: the unmasked range and the logarithm of the clamped depth.  The device's logf and the host's are each
    within 1 ulp of the logarithm (|log d| <= log 1000 < 8: an ulp of 4.8e-7), so the two may differ by 2 ulps; that passes
    through the normalisation times Dz / d_range, and the three rounded operations after it add 1.5 ulps of the result."""
    c, spec = "A", U.CASES["A"]
    S, Dz = spec["S"], spec["W"] // U.STRIDE
    depth = U.case_tensors(c, device=DEV)["rgbds"][0, :, 3]
    want_range = U.depth_range(depth.cpu(), True)
    d_near, d_far = tracker.depth_range(depth, True).tolist()
    assert want_range[0] < -6.9                                              # the clamped zeros: not masked in this form
    assert abs(d_near - want_range[0]) <= 2 * 4.8e-7 and abs(d_far - want_range[1]) <= 2 * 4.8e-7
    dm, zr = tracker.window_depth(depth[4:7], S, U.STRIDE, want_range[0], want_range[1], Dz, True)
    want, (lo, hi) = U.window_depth(depth[4:7].cpu().double(), S, U.STRIDE, want_range[0], want_range[1], Dz, True)
    bound = 2 * 4.8e-7 * Dz / (want_range[1] - want_range[0]) + 1.5 * float(np.spacing(np.float32(want.abs().max())))
    err = float((dm.cpu().double() - want).abs().max())
    print(f"log depth: max |window_depth - restatement64| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(zr, torch.stack([dm.min(), dm.max()])) and torch.equal(dm[3], dm[2])
    depth = depth.clone()
    depth[1, 4, 8] = float("nan")                                            # torch's min() and max() propagate it, and so do the kernels
    assert bool(torch.isnan(tracker.depth_range(depth, True)).all())
    assert (np.isfinite(tracker.depth_range(depth, False).tolist())).all()   # the mask does not select it
    dm, zr = tracker.window_depth(depth[:4], S, U.STRIDE, 0.5, 20.0, Dz, False)
    assert bool(torch.isnan(zr).all()) and int(torch.isnan(dm).sum()) == 1      # a sampled pixel


@pytest.mark.parametrize("c", list(U.CASES))
def test_sample_features_is_bit_equal_on_the_fixtures_maps(tracker, c):
    spec = U.CASES[c]
    first = torch.tensor(sorted(spec["first"]), device=DEV)
    seen_frames = set()
    for k, ind, prev, n in windows(c):
        if n == prev:
            continue
        coords = gpu(D[f"{c}.{k}.coords_init"])
        xy = coords[0, 0, prev:n]                                            # a [n, 3] row view
        got = tracker.sample_features(gpu(full_fmaps(c, k)), first[prev:n] - ind, xy)
        assert torch.equal(got.cpu(), torch.from_numpy(D[f"{c}.{k}.feat_init"])[0, 0, prev:n]), (c, k)
        seen_frames |= set((first[prev:n] - ind).tolist())
        h, w = spec["H"] // U.STRIDE, spec["W"] // U.STRIDE
        assert bool(((xy[:, 0] < 0) | (xy[:, 0] > w - 1) | (xy[:, 1] < 0) | (xy[:, 1] > h - 1)).any())          # clamped taps
    assert {0, spec["S"] - 1} <= seen_frames


@pytest.mark.parametrize("c", list(U.CASES))
def test_embed_conv_is_within_twice_the_gate(tracker, c):
    spec = U.CASES[c]
    S, h, w = spec["S"], spec["H"] // U.STRIDE, spec["W"] // U.STRIDE
    conv, gate = conv_of(c), float(D[f"gate.{c}.fmaps"])
    assert 0 < gate < 5e-4
    for k, ind, _, _ in windows(c):
        fr = U.computed_frames(k, S)
        fnet = gpu(U.fnet_maps(spec["seed"], k, fr.stop - fr.start, h, w))
        dm = gpu(D[f"{c}.{k}.dmaps"])[0, :, 0]
        zr = torch.stack([dm.min(), dm.max()])
        got = tracker.embed_conv(fnet, dm, zr, fr.start, conv, U.FREQS)
        err = float((got.cpu().double() - torch.from_numpy(D[f"{c}.{k}.fmaps"]).double()).abs().max())
        print(f"case {c} window {k}: max |embed_conv - ref32| {err:.3e}, gate {gate:.3e}")
        assert err <= 2 * gate, (c, k, err, gate)
        assert torch.equal(got, tracker.embed_conv(fnet, dm, zr, fr.start, conv, U.FREQS))         # bit-stable


def test_sliding_half_equals_the_full_window(tracker):
    c, spec = "A", U.CASES["A"]
    S, h, w = spec["S"], spec["H"] // U.STRIDE, spec["W"] // U.STRIDE
    conv = conv_of(c)
    fnet = gpu(U.fnet_maps(spec["seed"], 7, S, h, w))
    dm = gpu(D[f"{c}.1.dmaps"])[0, :, 0]
    zr = torch.stack([dm.min(), dm.max()])
    full = tracker.embed_conv(fnet, dm, zr, 0, conv, U.FREQS)
    window = torch.full_like(full, float("nan"))
    tracker.embed_conv(fnet[S // 2:], dm, zr, S // 2, conv, U.FREQS, out=window[S // 2:])
    assert torch.equal(window[S // 2:], full[S // 2:]) and bool(torch.isnan(window[:S // 2]).all())
    assert torch.equal(tracker.embed_conv(fnet.to(memory_format=torch.channels_last), dm, zr, 0, conv, U.FREQS), full)     # strides


def test_padding_is_zero_for_the_embedding_too(tracker):
    """Weights that are zero except on the cosine channels: cos(0) = 1, so a kernel that embedded its out-of-range taps (or
    a zero coordinate) instead of padding with zeros would be wrong by O(1) on the border."""
    c, spec = "C", U.CASES["C"]
    S, h, w = spec["S"], spec["H"] // U.STRIDE, spec["W"] // U.STRIDE
    conv = conv_of(c, "cpu")
    cosine = torch.zeros(U.C + U.EMB, dtype=torch.bool)
    for i in range(10):
        cosine[U.C + 3 + 6 * i + 3: U.C + 3 + 6 * i + 6] = True
    with torch.no_grad():
        conv.weight.mul_(cosine[None, :, None, None].float())
        conv.bias.zero_()
    dm = torch.from_numpy(D[f"{c}.0.dmaps"])[0, :, 0]
    zr = (dm.min(), dm.max())
    fnet = torch.zeros(S, U.C, h, w)
    want = U.embed_conv(fnet, dm, zr, 0, conv.weight, conv.bias)
    got = tracker.embed_conv(fnet.to(DEV), dm.to(DEV), torch.stack(zr).to(DEV), 0, conv.to(DEV), U.FREQS).cpu()
    err = float((got.double() - want.double()).abs().max())
    border = torch.ones(h, w, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    print(f"padding: max |kernel - restatement| {err:.3e}; border magnitude {float(want[..., border].abs().max()):.2f}")
    assert float(want[..., border].abs().max()) > 0.5                        # the border is where an O(1) miss would show
    assert err <= float(D[f"gate.{c}.fmaps"])


def test_constant_depth_gives_nan_maps(tracker):
    c, spec = "C", U.CASES["C"]
    S, h, w = spec["S"], spec["H"] // U.STRIDE, spec["W"] // U.STRIDE
    depth = torch.full((S, spec["H"], spec["W"]), 3.0, device=DEV)
    dm, zr = tracker.window_depth(depth, S, U.STRIDE, 0.5, 20.0, w)
    assert float(zr[0]) == float(zr[1])
    got = tracker.embed_conv(gpu(U.fnet_maps(1, 0, S, h, w)), dm, zr, 0, conv_of(c), U.FREQS)
    assert bool(torch.isnan(got).all())


def test_mid_shape_against_the_float64_restatement(tracker):
    """33 x 50 maps, S = 12, 64 queries: several tiles and several workgroups, ragged on both sides."""
    S, h, w, n = 12, 33, 50, 64
    g = torch.Generator().manual_seed(71)
    depth = (torch.rand(S, h * U.STRIDE, w * U.STRIDE, generator=g) * 19.5 + 0.5).to(DEV)
    fnet = torch.randn(S, U.C, h, w, generator=g).to(DEV)
    conv = conv_of("B")
    dm, zr = tracker.window_depth(depth, S, U.STRIDE, 0.5, 20.0, w)
    dm_ref, zr_ref = U.window_depth(depth.cpu(), S, U.STRIDE, 0.5, 20.0, w, False)
    assert torch.equal(dm.cpu(), dm_ref) and torch.equal(zr.cpu(), torch.stack(zr_ref))
    got = tracker.embed_conv(fnet, dm, zr, 0, conv, U.FREQS)
    want64 = U.embed_conv(fnet.double(), dm.double(), (zr[0].double(), zr[1].double()), 0, conv.weight.double(), conv.bias.double())
    want32 = U.embed_conv(fnet, dm, (zr[0], zr[1]), 0, conv.weight, conv.bias)
    own = float((want32.double() - want64).abs().max())
    err = float((got.double() - want64).abs().max())
    print(f"mid shape: max |embed_conv - restatement64| {err:.3e}; the float32 restatement's own error {own:.3e}")
    assert 0 < own < 5e-4 and err <= 2 * own

    frames = torch.randint(0, S, (n,), generator=g).to(torch.int32).to(DEV)
    frames[:2] = torch.tensor([0, S - 1], dtype=torch.int32)
    xy = torch.stack([torch.rand(n, generator=g) * (w + 6) - 3, torch.rand(n, generator=g) * (h + 6) - 3, torch.rand(n, generator=g)], -1).to(DEV)
    fm = got.contiguous()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    feats = tracker.sample_features(fm, frames, xy)
    torch.cuda.synchronize()
    added = torch.cuda.max_memory_allocated() - base
    assert added <= 2 * feats.numel() * 4, added                             # the reference's gather would be 54 MB here
    assert torch.equal(feats.cpu(), U.sample_features(fm.cpu(), frames.cpu(), xy.cpu()))


@pytest.mark.parametrize("c", list(U.CASES))
def test_forward_reproduces_the_reference(tracker, c):
    spec = U.CASES[c]

    def run(call):
        me = U.StandIn(c, torch.float32, DEV, U.embed3d_stand_in())
        T = U.case_tensors(c, device=DEV)
        with torch.no_grad():
            ret = call(me, T["rgbds"], T["queries"])
        return me, T, ret

    me, T, ret = run(lambda me, r, q: tracker.forward(me, r, q, iters=4))
    assert len(ret) == 7 and ret[6] is None and len(me.seen) == len(windows(c))
    assert (me.d_near, me.d_far, me.Dz) == (*D[f"{c}.d_range"], spec["W"] // U.STRIDE)
    for k, ind, prev, n in windows(c):
        seen = me.seen[k]
        fr = U.computed_frames(k, spec["S"])
        pieces = dict(seen, fmaps=seen["fmaps"][0, fr])
        for name in U.WINDOW_KEYS + ("fmaps",):
            got, want = pieces[name].cpu(), torch.from_numpy(D[f"{c}.{k}.{name}"])
            assert got.shape == want.shape and got.dtype == want.dtype, (c, k, name)
            if name in ("track_mask", "vis_init", "dmaps", "coords_init", "coords_dyn_init"):    # a mask, a copy, the bit-equal kernel, the correctly rounded divisions
                assert torch.equal(got, want), (c, k, name)
                continue
            gate = float(D[f"gate.{c}.{name}"])
            err = float((got.double() - want.double()).abs().max())
            print(f"case {c} window {k} {name}: max |forward - ref32| {err:.3e}, gate {gate:.3e}")
            assert err <= 2 * gate, (c, k, name, err, gate)
        if k:                                                                # the old half is carried, not recomputed
            assert torch.equal(seen["fmaps"][0, :spec["S"] // 2], me.seen[k - 1]["fmaps"][0, spec["S"] // 2:])
    named = dict(zip(U.RETURNS, ret))
    for name in ("traj_e", "depth_e", "traj_static_e"):
        assert torch.equal(named[name].cpu(), torch.from_numpy(D[f"{c}.{name}"])), (c, name)
    for name in ("vis_e", "dynamic_e"):
        assert float((named[name].cpu() - torch.from_numpy(D[f"{c}.{name}"])).abs().max()) <= 2.4e-7, (c, name)
    assert float((named["feat_init"].cpu().double() - torch.from_numpy(D[f"{c}.feat_init"]).double()).abs().max()) <= 2 * float(D[f"gate.{c}.feat_init"])
    assert np.array_equal(U.digest(T["rgbds"].cpu().numpy()), D[f"{c}.rgbds_digest"])       # normalised in place, as the reference does

    mod = types.ModuleType("stand_in_tracker")
    mod.MDTracker = type("MDTracker", (U.StandIn,), {"forward": lambda self, rgbds, queries: None})
    tracker.install(mod)

    def bound(me, r, q):
        me.__class__ = mod.MDTracker
        return me.forward(r, q, iters=4)
    me2, T2, ret2 = run(bound)
    for a, b in zip(ret[:6], ret2[:6]):
        assert torch.equal(a, b)
    assert torch.equal(T["rgbds"], T2["rgbds"])
