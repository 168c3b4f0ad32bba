"""-m gpu: the mono-depth alignment (bt_mono_align, include/batrack_depth.h, csrc/mono_align.hip) at its limits, through the C ABI
with raw pointers so that pointer offsets, NULL outputs and the workspace are the test's to choose.  The reference of every
comparison is numpy through the restatement (mono_util.py); equality is np.array_equal(..., equal_nan=True) with equal dtypes on
depth_out, frame_scale, frame_shift and aligns and plain equality on med_index.  No tolerance anywhere.
  constructed medians   frames whose middle pair of g, d, the ratio or g - s d parts at a chosen key byte (or is tied), stacked
                        into one scene a dtype and parity, on the vector path and on the scalar one (mono 4 bytes past 16)
  round P               element counts with gamma = 0, < 0.5, >= 0.5 and 0.7, neighbours at the two ranks that part at the first and
                        the last float32 byte, are tied or lie far apart (where numpy's two forms of lerp round differently), +inf from the
                        lower rank up, n = 1 and n = 2
  scene kernel          T = 65 .. 1100 with the chosen frame designed: every wave boundary, both 1024-trips, ties, a NaN frame
  grid-stride loops     the smallest scenes past every launch constant, from a workspace full of 0xFF
  pointers              mono / metric / out one element past 16 bytes, one at a time and together; the workspace 16 bytes into its
                        allocation and reused across scenes; all 16 patterns of NULL optional outputs
  the binding           float16 / bfloat16 / float64 mono_disp
Every output lies between 64 guard bytes of a pattern that must survive the call, and mono / metric must be left as found.
What each case reaches is asserted on the host by test_mono_limits_cpu.py."""
import functools
import itertools

import numpy as np
import pytest
import torch

from mono_util import (MEDIAN_HW, PERCENTILE_PAIRS, PERCENTILE_SHAPES, SCENE_T, STRIDE_SCENES, designed_scene, median_scene, percentile_scene, restate,
                       restate_frames, scene_designs, stride_scene)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [np.float32, np.float64]
GUARD, PATTERN = 64, 0xA5


def _lib():
    from batrack_amd import _lib as m
    return m, m.lib()


def carve(host, offset_bytes):
    """A device copy of `host` that starts offset_bytes past a 16-byte boundary.  Returns (address, owner, byte view)."""
    host = np.require(host, requirements="CW")                            # (a copy only of a shared, read-only array)
    raw = torch.zeros(host.nbytes + 64, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 16 == 0
    view = raw[offset_bytes:offset_bytes + host.nbytes]
    view.copy_(torch.from_numpy(host.view(np.uint8).reshape(-1)))
    return raw.data_ptr() + offset_bytes, raw, view


class Guarded:
    """nbytes of output that start offset_bytes past a 16-byte boundary, GUARD bytes of PATTERN on both sides (and inside, so an
    element the call leaves unwritten shows)."""

    def __init__(self, nbytes, offset_bytes=0):
        self.raw = torch.full((GUARD + offset_bytes + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 16 == 0 and GUARD % 16 == 0
        self.start, self.nbytes = GUARD + offset_bytes, nbytes
        self.ptr = self.raw.data_ptr() + self.start

    def read(self, dtype):
        assert bool((self.raw[:self.start] == PATTERN).all()) and bool((self.raw[self.start + self.nbytes:] == PATTERN).all()), "guard bytes overwritten"
        return self.raw[self.start:self.start + self.nbytes].cpu().numpy().view(dtype)


def workspace(T, hw, dt, fill=None, offset=0):
    _, L = _lib()
    nbytes = int(L.bt_mono_align_workspace_bytes(T, hw, dt))
    assert nbytes > 0
    ws = torch.zeros(nbytes + offset, dtype=torch.uint8, device=DEV)
    if fill is not None:
        ws.fill_(fill)
    return ws, ws.data_ptr() + offset


ALL = (True, True, True, True)


def raw_mono(d, m, mono_off=0, metric_off=0, out_off=0, want=ALL, ws=None, ws_fill=None, ws_off=0):
    """bt_mono_align on device copies of d [T, hw] float32 and m [T, hw]; the offsets in elements past a 16-byte boundary; `want`:
    which of frame_scale, frame_shift, aligns, med_index are passed (the others NULL); `ws`: (tensor, address) to reuse, otherwise
    a new workspace filled with ws_fill that starts ws_off bytes into its allocation.  Returns depth, s, c, aligns, k (None where
    NULL) after checking the guard bytes of every output and that the inputs are as they were."""
    lm, L = _lib()
    d, m = np.require(d, np.float32, "CW"), np.require(m, None, "CW")
    T, hw = m.shape[0], m[0].size
    es = m.dtype.itemsize
    dt = lm.BT_DEPTH_F64 if m.dtype == np.float64 else lm.BT_DEPTH_F32
    dp, _d_own, d_view = carve(d, 4 * mono_off)
    mp, _m_own, m_view = carve(m, es * metric_off)
    out = Guarded(T * hw * es, es * out_off)
    opt = [Guarded(T * es), Guarded(T * es), Guarded(3 * es), Guarded(8)]
    if ws is None:
        ws = workspace(T, hw, dt, ws_fill, ws_off)
    lm.check(L.bt_mono_align(dp, mp, T, hw, dt, out.ptr, *[o.ptr if w else None for o, w in zip(opt, want)], ws[1],
                             torch.cuda.current_stream().cuda_stream), "bt_mono_align")
    depth = out.read(m.dtype).reshape(m.shape)
    got = [o.read(np.int64 if i == 3 else m.dtype) for i, o in enumerate(opt)]
    for g, w, o in zip(got, want, opt):
        if not w:
            assert (g.view(np.uint8) == PATTERN).all()                    # a NULL output's stand-in is untouched
    assert bool((d_view == torch.from_numpy(d.view(np.uint8).reshape(-1)).to(DEV)).all()), "mono was written"
    assert bool((m_view == torch.from_numpy(m.view(np.uint8).reshape(-1)).to(DEV)).all()), "metric was written"
    s, c, al, k = (g if w else None for g, w in zip(got, want))
    return depth, s, c, al, None if k is None else int(k[0])


def assert_same(got, ref, what=""):
    """Every output present in `got` equals the reference's: dtype, shape, NaN places and the other elements' values; k plainly."""
    for name, a, b in zip(("depth", "frame_scale", "frame_shift", "aligns"), got[:4], ref[:4]):
        if a is None:
            continue
        b = np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if not np.array_equal(a, b, equal_nan=True):
            bad = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))).ravel())
            raise AssertionError((what, name, "first differing elements", bad[:8], a.ravel()[bad[:4]], b.ravel()[bad[:4]]))
    if got[4] is not None:
        assert got[4] == ref[4], (what, "med_index", got[4], ref[4])


def assert_same_bits(got, base, what=""):
    for a, b in zip(got[:4], base[:4]):
        if a is not None:
            assert a.tobytes() == b.tobytes(), what
    assert got[4] is None or got[4] == base[4], what


# ---------------------------------------------------------------------- constructed medians: the radix select
@pytest.mark.parametrize("hw", MEDIAN_HW)
@pytest.mark.parametrize("dtype", DTYPES)
def test_constructed_medians_are_numpy_medians_exactly(dtype, hw):
    """Frames of one launch part at different key bytes (mono_util.median_frames: every byte and a tie of g and d, the first and
    the last byte and a tie of the ratio and of g - s d, and what lies between), on an even and an odd count.  An upper selection
    that shared its lower one's histogram a pass too long, or left it a pass too soon, returns a neighbour of the middle pair."""
    d, m = median_scene(dtype, hw)
    assert len(d) >= 3
    ref = restate(d, m)
    assert not np.isnan(ref[1]).any() and not np.isnan(ref[2]).any()
    assert_same(raw_mono(d, m), ref, "aligned")                           # hw = 40: the vector path (A/B/C, P and the write)
    assert_same(raw_mono(d, m, mono_off=1), ref, "mono offset")           # the scalar path in every kernel


# ---------------------------------------------------------------------- round P
P_CASES = [(shape, kind) for shape in PERCENTILE_SHAPES for kind in PERCENTILE_PAIRS if kind != "inf" or shape == "gamma_low"]


@pytest.mark.parametrize("shape,kind", P_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_percentile_ranks_and_interpolation(dtype, shape, kind):
    """The 98th percentile of y = a_s d + a_c over all elements: numpy's two ranks, gamma and both forms of its lerp.  None of
    the element counts is a multiple of 4 but one, so the vector path's tail carries elements in round P and in the write."""
    d, m = percentile_scene(shape, kind, dtype)
    ref = restate(d, m)
    assert_same(raw_mono(d, m), ref, "aligned")
    assert_same(raw_mono(d, m, mono_off=1), ref, "mono offset")


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_and_two_elements(dtype):
    """n = 1: numpy's previous and next index are both -1 (the last element); n = 2: ranks 0 and 1."""
    for T, hw in ((1, 1), (1, 2), (2, 1)):
        d, m = stride_scene(T, hw, dtype, seed=7)
        ref = restate(d, m)
        assert np.isfinite(ref[3]).all()
        assert_same(raw_mono(d, m, ws_fill=0xFF), ref, (T, hw))
        assert_same(raw_mono(d, m, mono_off=1, metric_off=1, out_off=1), ref, (T, hw, "offset"))


# ---------------------------------------------------------------------- the scene kernel
@pytest.mark.parametrize("T", SCENE_T)
@pytest.mark.parametrize("dtype", DTYPES)
def test_scene_kernel_chooses_the_designed_frame(dtype, T):
    """k_ma_scene is one workgroup of kSceneThreads = 1024: frame t is lane t % 64 of wave (t % 1024) / 64, and frames from 1024 on
    take the second trip of the histogram loop and of the argmin loop.  T = 65 is the smallest scene with a frame outside wave 0,
    1025 the smallest with a second trip.  The chosen frame is designed (mono_util.scene_designs): at 0, in the last lane of wave
    0, the first of wave 1, at 1023, at 1024 and at T - 1; tied with a copy in another wave and in the other trip (the first
    wins); and with a NaN frame past 1024 (k = 0)."""
    ws = workspace(T, 4, 0 if dtype == np.float32 else 1, 0xFF)           # allocated once, reused dirty by every design
    for k, tie, nan_frame in scene_designs(T):
        d, m, ref = designed_scene(T, 4, dtype, k, tie, nan_frame)
        got = raw_mono(d, m, ws=ws)
        assert got[4] == ref[4] == (0 if nan_frame is not None else k), (k, tie, nan_frame, got[4], ref[4])
        assert_same(got, ref, (k, tie, nan_frame))


# ---------------------------------------------------------------------- grid-stride loops
@functools.lru_cache(maxsize=None)
def stride_case(T, hw, dtype):
    d, m = stride_scene(T, hw, dtype)
    ref = restate_frames(d, m)
    for x in (d, m) + tuple(ref[:4]):
        x.flags.writeable = False                                         # shared, left unchanged
    return d, m, ref


@pytest.mark.parametrize("name", STRIDE_SCENES)
def test_grid_stride_loops(name):
    """Each scene of mono_util.STRIDE_SCENES is the smallest that reaches its code (test_mono_limits_cpu.py asserts the thresholds
    beside the source's constants).  From a workspace full of 0xFF: a clear that stopped after one trip leaves histograms or
    selection state of all ones."""
    T, hw, dtype, offsets = STRIDE_SCENES[name]
    d, m, ref = stride_case(T, hw, dtype)
    assert_same(raw_mono(d, m, ws_fill=0xFF, **offsets), ref, name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scene_wave_reduction_on_random_scenes(dtype):
    """T = 65 .. 1100 as they fall (no design), a second seed: the median of p over more than one wave and trip."""
    for T in SCENE_T:
        d, m = stride_scene(T, 4, dtype, seed=11)
        assert_same(raw_mono(d, m, ws_fill=0xFF), restate_frames(d, m), T)


# ---------------------------------------------------------------------- pointers, the workspace, NULL outputs
@pytest.mark.parametrize("hw", [260, 259])
@pytest.mark.parametrize("dtype", DTYPES)
def test_offset_pointers_give_the_aligned_calls_bits(dtype, hw):
    """mono, metric and out one element past a 16-byte boundary (4 bytes, or 8 in float64), one at a time and together: every
    VEC = false path that is taken because of a pointer (vf, vs, vw in run) and not because of hw % 4."""
    d, m = stride_scene(5, hw, dtype, seed=5)
    ref = restate(d, m)
    base = raw_mono(d, m)
    assert_same(base, ref)
    for offs in itertools.product((0, 1), repeat=3):
        if any(offs):
            got = raw_mono(d, m, mono_off=offs[0], metric_off=offs[1], out_off=offs[2])
            assert_same_bits(got, base, offs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_offset_workspace_reused_across_scenes(dtype):
    """The workspace 16 bytes into its allocation (16-byte aligned, no more), full of 0xFF, then reused without clearing by a scene
    of another T (whose Scene and Seg records lie elsewhere in it) and by the first again."""
    a = stride_scene(70, 36, dtype, seed=1)
    b = stride_scene(9, 131, dtype, seed=2)
    ws = workspace(70, 36, 0 if dtype == np.float32 else 1, 0xFF, offset=16)
    assert ws[1] % 32 == 16
    for d, m in (a, b, a):
        assert_same(raw_mono(d, m, ws=ws), restate(d, m))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_pattern_of_null_outputs(dtype):
    """The optional outputs are independent: each of the 16 patterns gives the full call's depth_out and the full call's values in
    the outputs that are present."""
    d, m = stride_scene(6, 45, dtype, seed=9)
    ref = restate(d, m)
    full = raw_mono(d, m)
    assert_same(full, ref)
    for want in itertools.product((True, False), repeat=4):
        got = raw_mono(d, m, want=want, ws_fill=0xFF)
        assert [g is not None for g in got[1:]] == list(want)
        assert_same_bits(got, full, want)


# ---------------------------------------------------------------------- the binding's conversions
@pytest.mark.parametrize("mono_dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_binding_converts_mono_disp_to_float32(mono_dtype):
    from batrack_amd.mono_depth import align_mono_depth
    d, m = stride_scene(4, 33, np.float32, seed=13)
    dg = torch.as_tensor(d.astype(np.float64) * (1 + 1e-9), device=DEV).to(mono_dtype).reshape(4, 3, 11)
    mg = torch.as_tensor(m, device=DEV).reshape(4, 3, 11)
    out, s, c, al, k = align_mono_depth(dg, mg, return_stats=True)
    converted = dg.to(torch.float32).cpu().numpy()                        # exact for float16 / bfloat16, rounded once for float64
    assert mono_dtype != torch.float64 or (converted.astype(np.float64) != dg.cpu().numpy()).any()
    ref = restate(converted, mg.cpu().numpy())
    assert_same((out.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy(), al.cpu().numpy(), k), ref, mono_dtype)
