"""GPU half of the tracker's input preparation (bt_frame_prep in include/batrack_video.h, batrack_amd/frontend/video.py,
tracker.forward_frames) against the reference's fixture (tests/golden/video_prep.npz) and the restatement in
tests/video_util.py.  No bound here comes from the kernel under test: the gates are the reference's own float32-vs-float64
differences of the resize, stored in the fixture; the comparison is with the FLOAT64 run and the bound is twice the gate.
Everything else is bit-equality: with the restatement's float32 run on the CPU, between the routes, between the cached and the
uncached window.

Measured on an MI355X (information, not gates): max |ours - float64 run| beside the gate
    up 3.05e-5 4.24e-4   down 2.27e-6 2.03e-6   odd 3.26e-5 1.07e-3   same 0 0
"""
import numpy as np
import pytest
import torch

import tracker_window_util as TW
import video_util as U
from batrack_amd import _lib

pytestmark = pytest.mark.gpu

D = dict(np.load(U.GOLD))
DEV = "cuda:0"
ROUTES = ("python", "abi", "op")


@pytest.fixture(scope="module")
def video():
    from batrack_amd.frontend import video
    return video


@pytest.fixture(scope="module")
def tracker():
    from batrack_amd.frontend import tracker
    return tracker


def bits(t):
    return t.contiguous().view(torch.int32)


def run_prep(video, route, image, depth, size, normalise=False, log=False):
    if route == "python":
        return video.prepare_frames(image, depth, size, normalise, log)
    if route == "abi":
        rc, out, dr, __ = U.raw_frame_prep(image, depth, size, normalise, log)
        assert rc == _lib.BT_OK
        return out, dr
    out = torch.empty(image.shape[0], 4, *size, device=DEV)
    dr = torch.empty(image.shape[0], 2, device=DEV)
    ws = torch.zeros((_lib.lib().bt_frame_prep_workspace_bytes(image.shape[0], *size) + 3) // 4, dtype=torch.int32, device=DEV)
    _lib.torch_ops(strict=True).frame_prep(image, depth, normalise, log, ws, out, dr)
    return out, dr


@pytest.mark.parametrize("c", list(U.CASES))
def test_resize_is_within_twice_the_gate_on_every_route(video, c):
    t = U.case_tensors(c, device=DEV)
    image, depth = t["rgbds"][0, :, :3], t["rgbds"][0, :, 3]
    got = {route: run_prep(video, route, image, depth, U.SIZE) for route in ROUTES}
    rgbd = got["python"][0]
    assert tuple(rgbd.shape) == (U.CASES[c]["T"], 4, *U.SIZE) and rgbd.dtype == torch.float32 and rgbd.is_contiguous()
    want, gate = D[f"{c}.f64.rgbds"], float(D[f"gate.{c}"])
    err = float(np.abs(rgbd.cpu().numpy().astype(np.float64) - want).max())
    print(f"case {c}: max |ours - float64 run| {err:.3e}, gate {gate:.3e}")
    if c in U.RESIZING:
        assert 0 < gate < 5e-3 and err <= 2 * gate, (c, err, gate)
    else:
        assert gate == 0 and torch.equal(rgbd, t["rgbds"][0]) and np.array_equal(rgbd.cpu().numpy(), D[f"{c}.rgbds"])
    assert torch.equal(rgbd.cpu(), U.resize(t["rgbds"][0], U.SIZE))            # the header's arithmetic, bit for bit
    for route in ("abi", "op"):
        assert torch.equal(got[route][0], rgbd) and torch.equal(bits(got[route][1]), bits(got["python"][1])), route


@pytest.mark.parametrize("c", list(U.CASES))
def test_uint8_hwc_and_float32_chw_give_equal_bits(video, c):
    t = U.case_tensors(c, device=DEV)
    image, depth = t["rgbds"][0, :, :3].contiguous(), t["rgbds"][0, :, 3].contiguous()
    hwc = image.to(torch.uint8).permute(0, 2, 3, 1).contiguous()                # [T, H, W, 3] as a loader leaves it
    view = hwc.permute(0, 3, 1, 2)
    assert not view.is_contiguous() and view.stride(1) == 1
    for normalise in (False, True):
        a, da = video.prepare_frames(image, depth, U.SIZE, normalise)
        b, db = video.prepare_frames(view, depth, U.SIZE, normalise)
        assert torch.equal(a, b) and torch.equal(bits(da), bits(db))


def test_normalised_colours_at_the_identity_size_are_the_cpus(video):
    H, W = 16, 20
    colours = torch.arange(256, dtype=torch.float32).repeat(4)[: 3 * H * W].reshape(1, 3, H, W)   # every uint8 value
    colours = torch.cat([colours, colours.flip(-1) + 0.37], 0)                                   # and values that are no integers
    depth = torch.rand(2, H, W, generator=torch.Generator().manual_seed(3)) + 0.5
    got, __ = video.prepare_frames(colours.to(DEV), depth.to(DEV), (H, W), True)
    assert torch.equal(got[:, :3].cpu(), 2 * (colours / 255.0) - 1.0)           # the CPU divides by a scalar with one rounding
    assert torch.equal(got[:, :3].cpu(), U.normalise(colours)) and torch.equal(got[:, 3].cpu(), depth)


def test_prepare_frames_keeps_one_workspace_and_leaves_its_tickets_zero(video):
    t = U.case_tensors("up", device=DEV)
    image, depth = t["rgbds"][0, :, :3], t["rgbds"][0, :, 3]
    first, __ = video.prepare_frames(image, depth, U.SIZE)
    key = (0, torch.cuda.current_stream().cuda_stream, 4)
    ws = video._workspaces[key]
    for size in (U.SIZE, (5, 7), (40, 61)):
        again, __ = video.prepare_frames(image, depth, size)
        assert video._workspaces[key] is ws and int(ws[:4].abs().sum()) == 0    # no allocation, no memset: the one launch
    many, dm = video.prepare_frames(image[:1].expand(9, -1, -1, -1), depth[:1].expand(9, -1, -1), U.SIZE)   # more tickets: a workspace of its own
    assert video._workspaces[(0, key[1], 12)] is not ws and all(torch.equal(m, first[0]) for m in many) and bool((dm == dm[0]).all())
    assert torch.equal(video.prepare_frames(image, depth, U.SIZE)[0], first)
    with pytest.raises(RuntimeError, match="workspace must be"):
        _lib.torch_ops(strict=True).frame_prep(image, depth, True, False, torch.zeros(2, dtype=torch.int32, device=DEV),
                                               torch.empty(3, 4, *U.SIZE, device=DEV), torch.empty(3, 2, device=DEV))


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("c", list(U.CASES))
def test_depth_range_is_the_window_kernels(video, tracker, c, log):
    t = U.case_tensors(c, device=DEV)
    rgbd, dr = video.prepare_frames(t["rgbds"][0, :, :3], t["rgbds"][0, :, 3], U.SIZE, True, log)
    assert dr.shape == (U.CASES[c]["T"], 2)
    for f in range(rgbd.shape[0]):
        assert torch.equal(bits(dr[f]), bits(tracker.depth_range(rgbd[f: f + 1, 3], log))), f
        if not log:
            assert dr[f].tolist() == list(U.depth_range(rgbd[f, 3].cpu(), log)), f
    if not log:
        assert float(dr[:, 0].min()) > 0.01


@pytest.mark.parametrize("c", list(U.CASES))
def test_compute_sparse_tracks_against_the_reference(video, c):
    me = U.StandIn(c, torch.float32, DEV)
    t = U.case_tensors(c, device=DEV)
    before = t["rgbds"].clone()
    tracks, depths, vis, stats = video.compute_sparse_tracks(me, t["rgbds"], t["queries"])
    assert torch.equal(t["rgbds"], before) and len(me.seen) == 1 and me.seen[0]["iters"] == 4 and set(stats) == {"dynamic_e"}
    seen, gate = me.seen[0], float(D[f"gate.{c}"])
    assert tuple(seen["rgbds"].shape) == (1, U.CASES[c]["T"], 4, *U.SIZE)
    err = float(np.abs(seen["rgbds"][0].cpu().numpy().astype(np.float64) - D[f"{c}.f64.rgbds"]).max())
    assert err <= 2 * gate, (c, err, gate)
    got = dict(queries=seen["queries"], tracks=tracks, depths=depths, visibilities=vis, dynamic_e=stats["dynamic_e"])
    for name, v in got.items():                                                # downstream of the network: the reference's bits
        assert v.dtype == torch.float32 and np.array_equal(v.cpu().numpy(), D[f"{c}.{name}"]), name


def test_backward_tracking_over_a_longer_window_raises(video):
    t = U.case_tensors("same", device=DEV)
    me = U.StandIn("same", torch.float32, DEV, backward=True, S_slam=16)
    with pytest.raises(RuntimeError, match="backward tracking"):
        video.compute_sparse_tracks(me, t["rgbds"], t["queries"])
    assert me.seen == []
    me = U.StandIn("same", torch.float32, DEV, backward=False, S_slam=16)      # the branch is off: the same window runs
    video.compute_sparse_tracks(me, t["rgbds"], t["queries"])
    assert len(me.seen) == 1


# ------------------------------------------------------------------------------------------------------------ the window cache
S, SIZE, RAW = 4, (36, 72), (30, 50)          # 9 x 18 maps at stride 4


class FrameEncoder:
    """A frame-independent stand-in encoder: 128 maps at stride 4 from elementwise operations on slices, so that a frame's
    maps have the same bits whatever it is batched with.  Counts its calls and their frames."""

    def __init__(self):
        g = torch.Generator().manual_seed(17)
        self.w = (torch.rand(3, 128, 1, 1, generator=g) - 0.5).to(DEV)
        self.calls = []

    def __call__(self, x):
        self.calls.append(x.shape[0])
        a, b = x[:, :, ::4, ::4], x[:, :, 1::4, 2::4]
        return a[:, 0:1] * self.w[0] + b[:, 1:2] * self.w[1] + (a[:, 2:3] * b[:, 0:1]) * self.w[2]


def raw_frames(n, seed=29):
    g = torch.Generator().manual_seed(seed)
    image = torch.randint(0, 256, (n, RAW[0], RAW[1], 3), generator=g, dtype=torch.uint8).to(DEV).permute(0, 3, 1, 2)
    depth = (torch.rand(n, *RAW, generator=g) * 19.5 + 0.5).to(DEV)
    depth[:, 0, :3] = 0.0
    return image, depth


def test_window_frames_prepares_and_encodes_each_frame_once(video, monkeypatch):
    image, depth = raw_frames(14)
    enc, prepared = FrameEncoder(), []
    real = video.prepare_frames
    monkeypatch.setattr(video, "prepare_frames", lambda im, *a, **k: (prepared.append((im.shape[0], a[2])), real(im, *a, **k))[1])
    wf = video.WindowFrames(S, enc, size=SIZE)
    pushed = 0
    for burst in (1, 2, 5, 1, 1, 1, 1, 1, 1):
        for __ in range(burst):
            wf.push(image[pushed], depth[pushed])
            pushed += 1
        del prepared[:], enc.calls[:]
        rgbd, fmaps, drange = wf.window()
        new = min(burst, S)
        assert prepared == [(new, True)] and enc.calls == [new]                # one launch, one encoder call, the new frames only
        n = min(S, pushed)
        assert len(wf) == n and rgbd.shape == (n, 4, *SIZE) and fmaps.shape == (n, 128, 9, 18) and drange.shape == (2,)
        fresh, fresh_dr = real(image[pushed - n: pushed], depth[pushed - n: pushed], SIZE, True)
        assert torch.equal(rgbd, fresh) and torch.equal(fmaps, FrameEncoder()(fresh[:, :3]))
        assert drange.tolist() == [float(fresh_dr[:, 0].min()), float(fresh_dr[:, 1].max())] and drange.is_cuda
    assert pushed == 14


def _tracker_stand_in(enc):
    me = TW.StandIn("C", torch.float32, DEV, TW.embed3d_stand_in())            # S = 4, stride 4, a real embedConv
    me.fnet = enc
    return me


@pytest.mark.parametrize("n", [3, 4])
def test_forward_frames_is_forward_on_the_stacked_frames(video, tracker, n):
    every_image, every_depth = raw_frames(6, seed=31)
    image, depth = every_image[6 - n:], every_depth[6 - n:]
    g = torch.Generator().manual_seed(41)
    queries = torch.stack([torch.tensor([0.0, float(n - 1), 1.0]), torch.rand(3, generator=g) * SIZE[1], torch.rand(3, generator=g) * SIZE[0],
                           torch.rand(3, generator=g) * 10 + 1], -1)[None].to(DEV)

    wf = video.WindowFrames(S, FrameEncoder(), size=SIZE)
    for f in range(6):                                                          # the window has slid before the call
        wf.push(every_image[f], every_depth[f])
        if f == 6 - n - 1:
            wf.clear() if n < S else wf.window()
    cached = _tracker_stand_in(wf.fnet)
    got = tracker.forward_frames(cached, wf, queries.clone(), iters=4)
    assert len(wf) == n

    rgbd, __ = video.prepare_frames(image, depth, SIZE, normalise=False)
    if n < S:
        rgbd = torch.cat([rgbd, rgbd[-1:].expand(S - n, -1, -1, -1)], 0)        # as get_window_trajs pads
    plain = _tracker_stand_in(FrameEncoder())
    want = tracker.forward(plain, rgbd[None].clone(), queries.clone(), iters=4)

    assert plain.fnet.calls == [S] and len(plain.seen) == len(cached.seen) == 1
    for k, v in plain.seen[0].items():
        assert torch.equal(cached.seen[0][k], v), k
    assert (cached.d_near, cached.d_far, cached.Dz) == (plain.d_near, plain.d_far, plain.Dz)
    assert len(got) == len(want) == 7 and got[6] is None and want[6] is None
    for a, b in zip(got[:6], want[:6]):
        assert a.shape == b.shape and a.shape[1] == S and torch.equal(a, b)
