"""k_frame_prep at its limits (batrack_amd/csrc/video_prep.hip, include/batrack_video.h): sizes of one row, one column and one
pixel; output widths and heights either side of the lane's vector (BT_VIDEO_VEC = 4 columns) and of the block's tile
(BT_VIDEO_TILE = 1024 pixels, 256 groups of four); more groups than BT_VIDEO_MAX_BLOCKS blocks cover in one trip; more frames
than the grid's frame dimension (BT_VIDEO_GRID_FRAMES = 64); an output pointer off the 16-byte grid; strided views; a frame
alone and in a batch; NaN and infinity in the depth; the mask at 0.01f and its successor; a workspace that is never zeroed
again; guard rows.  The expected values are the restatement's float32 run on the CPU (tests/video_util.py), bit for bit, and
`tracker.depth_range` on the returned plane.  Tiny shapes; nothing here provokes a fault, and refusals are return codes."""
import numpy as np
import pytest
import torch

import video_util as U
from batrack_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN_BITS = 0x7FC00000


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


def frames(F, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    image = torch.randint(0, 256, (F, 3, H, W), generator=g).float()
    depth = torch.rand(F, H, W, generator=g) * 19.5 + 0.5
    depth.view(-1)[:: 7] = 0.0
    return image, depth


def expected(image, depth, size, normalise):
    rgbd = U.resize(torch.cat([image.float(), depth[:, None]], 1), size)
    if normalise:
        rgbd[:, :3] = U.normalise(rgbd[:, :3])
    return rgbd


def check(video, tracker, image, depth, size, normalise=True, log=False):
    """prepare_frames on the GPU against the restatement and `tracker.depth_range`; returns (rgbd, drange)."""
    rgbd, dr = video.prepare_frames(image.to(DEV), depth.to(DEV), size, normalise, log)
    want = expected(image.cpu(), depth.cpu(), size, normalise)
    got = rgbd.cpu()                                             # a NaN equals a NaN (the CPU's default NaN has the sign bit set)
    assert got.shape == want.shape and bool(((bits(got) == bits(want)) | (torch.isnan(got) & torch.isnan(want))).all())
    for f in range(rgbd.shape[0]):
        assert torch.equal(bits(dr[f]), bits(tracker.depth_range(rgbd[f: f + 1, 3], log))), f
    return rgbd, dr


@pytest.mark.parametrize("H,W,oh,ow", [(1, 1, 1, 1), (1, 1, 3, 5), (1, 7, 1, 7), (1, 7, 2, 3), (1, 7, 1, 12), (6, 1, 6, 1), (6, 1, 3, 2), (6, 1, 9, 1),
                                         (5, 7, 1, 1), (5, 7, 1, 9), (5, 7, 6, 1)])
def test_one_row_one_column_one_pixel(video, tracker, H, W, oh, ow):
    image, depth = frames(2, H, W, seed=H * 100 + W)
    check(video, tracker, image, depth, (oh, ow))
    check(video, tracker, image, depth, (oh, ow), normalise=False, log=True)


@pytest.mark.parametrize("oh,ow", [(5, 3), (5, 4), (5, 5), (3, 8), (1, 1020), (1, 1023), (1, 1024), (1, 1025), (1, 1028),
                                     (255, 4), (256, 4), (257, 4), (257, 3), (13, 80), (13, 79)])
def test_output_sizes_either_side_of_the_vector_and_the_tile(video, tracker, oh, ow):
    image, depth = frames(2, 9, 11, seed=oh * 31 + ow)
    groups = oh * ((ow + U.VEC - 1) // U.VEC)
    assert U.blocks(oh, ow) == (groups + 255) // 256
    check(video, tracker, image, depth, (oh, ow))


def test_more_groups_than_one_trip_of_the_blocks_covers(video, tracker):
    oh, ow = 513, 2052                                           # 513 * 513 = 263169 groups: 1024 blocks of 256 lanes, and a second trip
    assert oh * (ow // U.VEC) > U.MAX_BLOCKS * 256 and U.blocks(oh, ow) == U.MAX_BLOCKS
    image, depth = frames(1, 6, 10, seed=5)
    rgbd, dr = check(video, tracker, image, depth, (oh, ow), normalise=False)
    assert dr[0].tolist() == list(U.depth_range(rgbd[0, 3].cpu(), False))


@pytest.mark.parametrize("H,W,oh,ow", [(1, 1 << 20, 1, 1100), (1 << 20, 1, 1100, 1), (1, 1 << 20, 2, 1027)])
def test_the_64_bit_coordinate(video, tracker, H, W, oh, ow):
    """(2 n_out + 1) n_in passes 2^31, so the launch is k_frame_prep<false>: 64-bit integers; 2 n_out is far below 2^24, so the
    quotient is still the float32 one of exact operands and the restatement's bits hold."""
    assert (2 * max(oh, ow) + 1) * max(H, W) >= 1 << 31 and 2 * max(oh, ow) < 1 << 24
    image, depth = frames(1, H, W, seed=37)
    check(video, tracker, image, depth, (oh, ow))


def test_an_output_pointer_off_the_16_byte_grid(video):
    image, depth = frames(3, 10, 14, seed=7)
    image, depth = image.to(DEV), depth.to(DEV)
    size = (12, 16)
    aligned, dr = video.prepare_frames(image, depth, size)
    assert aligned.data_ptr() % 16 == 0
    for shift in (1, 2, 3):
        buf = torch.full((aligned.numel() + 8,), -7.0, device=DEV)
        out = buf[shift: shift + aligned.numel()].view(aligned.shape)
        assert out.data_ptr() % 16 == 4 * shift
        got, dr2 = video.prepare_frames(image, depth, size, out=out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(got, aligned) and torch.equal(bits(dr2), bits(dr))
        assert bool((buf[:shift] == -7.0).all()) and bool((buf[shift + aligned.numel():] == -7.0).all())


def test_strided_views_are_read_in_place(video, tracker):
    g = torch.Generator().manual_seed(11)
    big = torch.randint(0, 256, (3, 40, 45, 3), generator=g, dtype=torch.uint8).to(DEV)          # HWC, then every second row and third column
    view = big.permute(0, 3, 1, 2)[1:, :, 3::2, 1::3]
    dbig = (torch.rand(5, 40, 45, generator=g) * 10 + 0.5).to(DEV)
    dview = dbig[1::2, 3::2, 1::3]
    assert view.shape == (2, 3, 19, 15) and dview.shape == (2, 19, 15) and not view.is_contiguous() and not dview.is_contiguous()
    a, da = video.prepare_frames(view, dview, (17, 20))
    b, db = check(video, tracker, view.float().contiguous().cpu(), dview.contiguous().cpu(), (17, 20))
    assert torch.equal(a, b) and torch.equal(bits(da), bits(db))
    rc, c, dc, __ = U.raw_frame_prep(view, dview, (17, 20), normalise=True)
    assert rc == _lib.BT_OK and torch.equal(c, a) and torch.equal(bits(dc), bits(da))
    # a broadcast frame (stride 0) is a view too
    e, de = video.prepare_frames(view[:1].expand(3, -1, -1, -1), dview[:1].expand(3, -1, -1), (17, 20))
    assert all(torch.equal(e[i], a[0]) and torch.equal(bits(de[i]), bits(da[0])) for i in range(3))


def test_one_frame_and_more_frames_than_the_grid_has(video, tracker):
    F = U.GRID_FRAMES + 3
    image, depth = frames(F, 5, 6, seed=13)
    depth[F - 1] = 0.0                                           # a frame with nothing above the mask, in the second trip
    rgbd, dr = check(video, tracker, image, depth, (7, 9))
    assert dr[F - 1].tolist() == [float("inf"), float("-inf")]
    for f in (0, U.GRID_FRAMES - 1, U.GRID_FRAMES, F - 1):       # alone: the same bits
        one, dr1 = video.prepare_frames(image[f: f + 1].to(DEV), depth[f: f + 1].to(DEV), (7, 9))
        assert torch.equal(one[0], rgbd[f]) and torch.equal(bits(dr1[0]), bits(dr[f])), f


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("size", [(9, 11), (14, 17), (5, 6)])
def test_a_nan_or_an_infinity_reaches_the_pixels_whose_taps_touch_it(video, tracker, value, size):
    H, W, y, x = 9, 11, 4, 6
    image, depth = frames(2, H, W, seed=17)
    depth[1, y, x] = value
    for log in (False, True):
        rgbd, dr = check(video, tracker, image, depth, size, log=log)
        hit = U.touched(H, size[0], y)[:, None] & U.touched(W, size[1], x)[None, :]
        assert int(hit.sum()) >= 1
        assert torch.equal(~torch.isfinite(rgbd[1, 3].cpu()), hit) and bool(torch.isfinite(rgbd[0]).all()) and bool(torch.isfinite(rgbd[1, :3]).all())
        # `check` has compared drange with bt_depth_range on the plane; what that propagates, from the plane on the CPU: the
        # mask never selects a NaN, an infinity above it is the maximum, and with the logarithm a NaN makes both NaN
        same = lambda a, b: (a != a and b != b) or a == b or (log and np.isfinite(a) and np.isfinite(b))
        assert all(same(a, b) for a, b in zip(dr[1].tolist(), U.depth_range(rgbd[1, 3].cpu(), log))), (dr[1].tolist(), log)
        if not log:
            assert not bool(torch.isnan(dr[1]).any())
        assert torch.isfinite(dr[0]).all()


def test_the_mask_is_pinned_at_0_01(video):
    at = float(np.float32(0.01))
    above = float(np.nextafter(np.float32(0.01), np.float32(1)))
    image, depth = frames(3, 6, 8, seed=19)
    depth[0] = torch.tensor([0.0, at, 0.009, -3.0]).repeat(12).reshape(6, 8)
    depth[1] = depth[0]
    depth[1, 5, 7] = above
    depth[2] = depth[1]
    depth[2, 0, 0] = 5.0
    rgbd, dr = video.prepare_frames(image.to(DEV), depth.to(DEV), (6, 8))       # the identity size: the values as they are
    assert torch.equal(rgbd[:, 3].cpu(), depth)
    inf = float("inf")
    assert dr.tolist() == [[inf, -inf], [above, above], [above, 5.0]]
    __, drl = video.prepare_frames(image.to(DEV), depth.to(DEV), (6, 8), use_log_depth=True)
    want = torch.log(depth.clamp(min=1e-3))
    assert torch.allclose(drl.cpu(), torch.stack([want.amin((1, 2)), want.amax((1, 2))], -1), rtol=1e-6, atol=0)


def test_a_workspace_with_nan_partials_is_reused_without_zeroing(video, tracker):
    F, size = 3, (40, 61)                                        # 40 * 16 = 640 groups: three blocks a frame
    assert U.blocks(*size) == 3
    words = U.workspace_bytes(F, *size) // 4
    assert _lib.lib().bt_frame_prep_workspace_bytes(F, *size) == 4 * words
    ws = torch.full((words,), NAN_BITS, dtype=torch.int32, device=DEV)
    ws[:4] = 0                                                   # the tickets, zero on entry; every partial a NaN
    for trip in range(4):
        image, depth = frames(F, 23, 31, seed=100 + trip)
        if trip == 2:
            depth[1] = 0.0
        log = trip == 3
        rc, rgbd, dr, __ = U.raw_frame_prep(image.to(DEV), depth.to(DEV), size, normalise=True, log=log, ws=ws)
        assert rc == _lib.BT_OK and ws[:4].tolist() == [0, 0, 0, 0], trip
        assert torch.equal(bits(rgbd.cpu()), bits(expected(image, depth, size, True)))
        for f in range(F):
            assert torch.equal(bits(dr[f]), bits(tracker.depth_range(rgbd[f: f + 1, 3], log))), (trip, f)
        if trip == 2:
            assert dr[1].tolist() == [float("inf"), float("-inf")]
        assert bool(torch.isfinite(ws[4:].view(torch.float32)).all()) or trip == 2     # the pairs were all rewritten


def test_guard_rows_stay_untouched(video):
    F, size = 2, (10, 13)
    image, depth = frames(F, 7, 9, seed=23)
    n = F * 4 * size[0] * size[1]
    buf = torch.full((n + 2 * 64,), -5.0, device=DEV)
    drbuf = torch.full((F + 2, 2), -5.0, device=DEV)
    rc, rgbd, dr, __ = U.raw_frame_prep(image.to(DEV), depth.to(DEV), size, normalise=True, out=buf[64: 64 + n].view(F, 4, *size), drange=drbuf[1: 1 + F])
    assert rc == _lib.BT_OK
    assert bool((buf[:64] == -5.0).all()) and bool((buf[64 + n:] == -5.0).all())
    assert bool((drbuf[0] == -5.0).all()) and bool((drbuf[-1] == -5.0).all()) and bool((drbuf[1:-1] > 0).all())
    assert torch.equal(bits(rgbd.cpu()), bits(expected(image, depth, size, True)))


def test_refusals_are_return_codes_and_launch_nothing(video):
    image, depth = frames(2, 7, 9, seed=29)
    image, depth = image.to(DEV), depth.to(DEV)
    out = torch.full((2, 4, 5, 6), -3.0, device=DEV)
    dr = torch.full((2, 2), -3.0, device=DEV)
    L = _lib.lib()
    ws = torch.zeros(64, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    args = lambda **k: (k.get("image", image.data_ptr()), 0, *k.get("si", image.stride()), depth.data_ptr(), *k.get("sd", depth.stride()),
                        k.get("F", 2), 7, 9, k.get("oh", 5), k.get("ow", 6), 1, 0, ws.data_ptr(), out.data_ptr(), dr.data_ptr(), stream)
    assert L.bt_frame_prep(*args(image=None)) == _lib.BT_EINVAL
    assert L.bt_frame_prep(*args(oh=0)) == _lib.BT_EINVAL and L.bt_frame_prep(*args(si=(189, 63, -9, 1))) == _lib.BT_EINVAL
    assert L.bt_frame_prep(*args(si=(1 << 31, 63, 9, 1))) == _lib.BT_EUNSUPPORTED
    assert L.bt_frame_prep(*args(oh=1 << 31)) == _lib.BT_EUNSUPPORTED and L.bt_frame_prep(*args(F=0)) == _lib.BT_OK
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((dr == -3.0).all()) and int(ws.abs().sum()) == 0
    with pytest.raises(RuntimeError, match="uint8 or float32"):
        video.prepare_frames(image.double(), depth)
    with pytest.raises(RuntimeError, match=r"\[F, 3, H, W\]"):
        video.prepare_frames(image[:, :2], depth)
    with pytest.raises(RuntimeError, match="`out` must be"):
        video.prepare_frames(image, depth, (5, 6), out=out[:, :, :, ::2])
    empty, dre = video.prepare_frames(image[:0], depth[:0], (5, 6))
    assert empty.shape == (0, 4, 5, 6) and dre.shape == (0, 2)
