"""CPU half of the fused correlation lookup (include/batrack_corr.h): the reference's fixture
(tests/golden/corr_lookup.npz, made by its unmodified CorrBlock) against the numpy restatement of the header's formula
in tests/corr_util.py; the ABI's refusals, the exported symbols, the operators' schemas, CorrBlock's signatures, the
CPU-tensor error, install() and the import surface — none of which touch a GPU."""
import ctypes
import inspect
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import corr_util
from batrack_amd import _lib

D = dict(np.load(corr_util.GOLD))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=list(corr_util.CASES))
def case(request):
    c = request.param
    fmaps, targets, coords3, spec = corr_util.load_case(c)
    return c, fmaps, targets, coords3, spec


def test_generator_reproduces_the_fixtures_inputs(case):
    c, fmaps, targets, coords3, spec = case
    assert list(D[f"{c}.spec"]) == [spec[k] for k in ("seed", "S", "C", "H", "W", "N", "L", "r")]
    for name, a in (("fmaps", fmaps), ("targets", targets), ("coords3", coords3)):
        assert np.array_equal(corr_util.digest(a[None]), D[f"{c}.digest.{name}"]), name
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))                   # float32 values


def test_specification_reproduces_the_reference(case):
    """float64 restatement against the reference's float64 run, stored as the float32 it returns: half a float32 unit in
    the last place per entry.  Pins the window order, the level scaling, the zero padding, the pooling of odd sizes."""
    c, fmaps, targets, coords3, spec = case
    ref = D[f"{c}.ref"].astype(np.float64)
    got = corr_util.np_corr_lookup(fmaps, targets, coords3[..., :2], spec["L"], spec["r"])
    assert got.shape == ref.shape == (spec["S"], spec["N"], spec["L"] * (2 * spec["r"] + 1) ** 2)
    excess = np.abs(got - ref) - (6e-8 * np.abs(ref) + 1e-12)
    assert excess.max() <= 0, (excess.max(), np.abs(got - ref).max())
    # the natural order (first index moves y) is a different function: the fixture tells them apart
    d = 2 * spec["r"] + 1
    swapped = got.reshape(*got.shape[:2], spec["L"], d, d).transpose(0, 1, 2, 4, 3).reshape(got.shape)
    assert np.abs(swapped - ref).max() > 0.1


def test_float32_restatement_stays_within_the_gate(case):
    c, fmaps, targets, coords3, spec = case
    gate = float(D[f"gate.{c}"])
    assert 0 < gate < 1e-4
    got = corr_util.np_corr_lookup(fmaps, targets, coords3[..., :2], spec["L"], spec["r"], np.float32)
    assert got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - D[f"{c}.ref"].astype(np.float64)).max()
    assert err <= gate, (err, gate)


def test_fixture_cases_cover_what_they_claim(case):
    c, fmaps, targets, coords3, spec = case
    H, W, N, r, L = spec["H"], spec["W"], spec["N"], spec["r"], spec["L"]
    x, y = coords3[..., 0], coords3[..., 1]
    outside = (x < 0) | (x > W - 1) | (y < 0) | (y > H - 1)
    assert 0.08 < outside.mean() < 0.25
    near = outside & (x >= -8) & (x <= W + 7) & (y >= -8) & (y <= H + 7)
    assert near.sum() >= outside.sum() - spec["S"]                                           # all but the far one a frame
    assert (x[:, 0] == 0).all() and (y[:, 0] == 0).all() and (x[:, 1] == W - 1).all() and (y[:, 1] == H - 1).all()
    assert (x[:, 2] == -40).all() and not D[f"{c}.ref"][:, 2].any()                          # an all-zero window
    assert D[f"{c}.ref"][:, 0].any() and D[f"{c}.ref"][:, 1].any()
    q = coords3[:, 3:corr_util.N_SPECIAL, :2] * 4
    assert np.array_equal(q, np.round(q))                                                    # quarter-pixel positions
    assert ((H % 2 == 1) and (W % 2 == 1)) == (c == "b")                                     # odd sizes: the pooling floors
    assert corr_util.level_sizes(45, 61, 3) == [(45, 61), (22, 30), (11, 15)]
    assert [f.shape[-2:] for f in corr_util.np_pyramid(fmaps, L)] == corr_util.level_sizes(H, W, L)
    assert coords3.shape[-1] == 3                                                            # handed over as a [..., :2] view


def test_fixture_stays_small():
    assert os.path.getsize(corr_util.GOLD) < 523 * 1024


def test_symbols_are_exported_and_sources_listed():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("bt_corr_pyramid_bytes", "bt_corr_pyramid", "bt_corr_lookup"):
        assert hasattr(L, name), name
    assert "corr_lookup.hip" in _lib.SOURCES
    assert any(h.endswith("batrack_corr.h") for h in _lib.HEADERS)
    header = open(os.path.join(ROOT, "include", "batrack_corr.h")).read()
    for name in ("bt_corr_pyramid_bytes", "bt_corr_pyramid", "bt_corr_lookup", "FIRST window index"):
        assert name in header, name
    assert "correlation lookup" in _lib.ERRORS[_lib.BT_EUNSUPPORTED]


def test_pyramid_bytes():
    L = _lib.lib()
    for spec in corr_util.CASES.values():
        S, C = spec["S"], spec["C"]
        want = 4 * C * S * sum(h * w for h, w in corr_util.level_sizes(spec["H"], spec["W"], spec["L"]))
        assert L.bt_corr_pyramid_bytes(S, C, spec["H"], spec["W"], spec["L"]) == want
    assert L.bt_corr_pyramid_bytes(12, 128, 96, 128, 4) == 4 * 128 * 12 * (12288 + 3072 + 768 + 192)
    assert L.bt_corr_pyramid_bytes(1, 130, 8, 8, 1) == 0 and L.bt_corr_pyramid_bytes(1, 128, 8, 8, 9) == 0


def test_abi_refuses_before_launching():
    """Argument checks return their codes before anything is enqueued (no GPU needed: nothing is launched)."""
    L = _lib.lib()
    p = ctypes.c_void_p(256)                           # never dereferenced: every call below is refused first
    EINVAL, EUNS = _lib.BT_EINVAL, _lib.BT_EUNSUPPORTED
    ok = dict(fmaps=p, S=2, C=128, H=16, W=16, levels=4, pyr=p)
    pyramid = lambda **k: L.bt_corr_pyramid(*(dict(ok, **k)[n] for n in ok), None)
    ok2 = dict(pyr=p, S=2, C=128, H=16, W=16, levels=4, radius=3, targets=p, coords=p, cstride=2, N=8, out=p)
    lookup = lambda **k: L.bt_corr_lookup(*(dict(ok2, **k)[n] for n in ok2), None)
    for name in ("fmaps", "pyr"):
        assert pyramid(**{name: None}) == EINVAL, name
    for name in ("pyr", "targets", "coords", "out"):
        assert lookup(**{name: None}) == EINVAL, name
    for call in (pyramid, lookup):
        for name in ("S", "C", "H", "W", "levels"):
            assert call(**{name: 0}) == EINVAL, name
            assert call(**{name: -1}) == EINVAL, name
        assert call(C=126) == EINVAL                   # C % 4
        assert call(levels=6) == EINVAL                # 16 >> 5 is an empty map
        assert call(C=516) == EUNS
        assert call(levels=9, H=1024, W=1024) == EUNS
        assert call(H=32769) == EUNS
    assert lookup(N=-1) == EINVAL
    assert lookup(radius=-1) == EINVAL
    assert lookup(cstride=1) == EINVAL
    assert lookup(radius=8) == EUNS
    assert lookup(N=(1 << 31) // 8) == EUNS            # S * N * levels work items: 32-bit index arithmetic
    assert lookup(N=(1 << 31) // 8 - 1, coords=None) == EINVAL
    assert lookup(N=0) == _lib.BT_OK                   # nothing to do, nothing launched
    assert lookup(N=0, cstride=3, radius=7, C=512, levels=1) == _lib.BT_OK


def test_operator_schemas():
    ops = _lib.torch_ops(strict=True)
    assert str(ops.corr_pyramid.default._schema) == "batrack_hip::corr_pyramid(Tensor fmaps, int levels) -> Tensor"
    assert str(ops.corr_lookup.default._schema) == ("batrack_hip::corr_lookup(Tensor pyramid, int[] shape, int levels, int radius, "
                                                    "Tensor targets, Tensor coords) -> Tensor")


def test_corrblock_has_the_references_signatures():
    from batrack_amd.frontend.corr import CorrBlock
    got = [str(inspect.signature(f)) for f in (CorrBlock.__init__, CorrBlock.corr, CorrBlock.sample)]
    assert got == list(D["signatures"])
    assert got[0] == "(self, fmaps, num_levels=4, radius=4)"


def test_cpu_tensors_raise():
    from batrack_amd.frontend.corr import CorrBlock
    with pytest.raises(RuntimeError, match="GPU"):
        CorrBlock(torch.zeros(1, 2, 8, 16, 16), num_levels=2, radius=1)
    blk = object.__new__(CorrBlock)
    blk.S, blk.C, blk.H, blk.W, blk.B, blk.num_levels, blk.radius, blk.targets = 2, 8, 16, 16, 1, 2, 1, None
    with pytest.raises(RuntimeError, match="GPU"):
        blk.corr(torch.zeros(1, 2, 4, 8))
    with pytest.raises(RuntimeError, match="GPU"):
        blk.sample(torch.zeros(1, 2, 4, 2))
    ops = _lib.torch_ops(strict=True)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.corr_pyramid(torch.zeros(2, 8, 16, 16), 2)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.corr_lookup(torch.zeros(2 * 8 * (256 + 64)), [2, 8, 16, 16], 2, 1, torch.zeros(2, 4, 8), torch.zeros(2, 4, 2))


def test_install_swaps_the_name_and_returns_the_old_one():
    from batrack_amd.frontend import corr
    tracker = types.ModuleType("stand_in_tracker")
    old = type("CorrBlock", (), {})
    tracker.CorrBlock = old
    assert corr.install(tracker) is old
    assert tracker.CorrBlock is corr.CorrBlock
    assert corr.install(tracker) is corr.CorrBlock     # a second call finds this class


def test_import_surface():
    """batrack_amd.frontend does not import oracle; importing batrack_amd does not import the front end, and importing
    the front end loads no native library."""
    code = ("import sys; import batrack_amd; assert not any(m.startswith('batrack_amd.frontend') for m in sys.modules); "
            "import batrack_amd.frontend.corr; from batrack_amd import _lib; "
            "assert 'oracle' not in sys.modules and _lib._lib is None and _lib._torch_ops is None; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


@pytest.mark.parametrize("C,r,L,H,W", [(16, 3, 4, 48, 64), (16, 4, 3, 45, 61), (8, 7, 3, 4, 4), (8, 3, 4, 8, 8), (8, 2, 1, 1, 37)])
def test_restatement_agrees_with_the_volume_formulation_on_the_edge_inputs(C, r, L, H, W):
    """What tests/test_gpu_corr_limits.py leans on.  On the planted coordinates of corr_util.edge_queries the float64
    restatement and the float64 volume formulation agree to 1e-12 wherever both are defined (finite coordinates, levels
    more than one pixel high and wide); a level one pixel high or wide is NaN in the volume formulation (it divides by
    W_l - 1 = 0) and finite in the restatement; a query with a non-finite coordinate is NaN in every output of the volume
    formulation; a far query is exactly 0 in both; the first integer positions wholly outside are exactly 0 at level 0."""
    S, N, d = 2, 64, 2 * r + 1
    fmaps, targets, coords, kinds, calm = corr_util.planted_inputs(41 + C + H, S, C, H, W, N, r)
    nonfinite = kinds == "nonfinite"
    assert np.array_equal(nonfinite, ~np.isfinite(coords).all((0, 2))) and nonfinite.sum() == 11
    with np.errstate(all="ignore"):
        vol = corr_util.volume_lookup_cpu64(fmaps, targets, coords, L, r).reshape(S, N, L, d * d)
    ref = corr_util.np_corr_lookup(fmaps, targets, np.where(nonfinite[None, :, None], calm, coords), L, r).reshape(S, N, L, d * d)
    assert np.isfinite(ref).all()
    sizes = corr_util.level_sizes(H, W, L)
    thin = np.array([min(h, w) == 1 for h, w in sizes])              # levels one pixel high or wide
    assert thin.any() == (min(sizes[-1]) == 1)
    assert np.isnan(vol[:, :, thin]).all()                            # every output of such a level, for every query
    assert np.isnan(vol[:, nonfinite]).all()                          # at every level
    assert not np.isnan(vol[:, ~nonfinite][:, :, ~thin]).any()
    both = vol[:, ~nonfinite][:, :, ~thin], ref[:, ~nonfinite][:, :, ~thin]
    if both[0].size:
        assert np.abs(both[0] - both[1]).max() <= 1e-12, np.abs(both[0] - both[1]).max()
    far = kinds == "far"
    assert far.sum() == 22 and not ref[:, far].any() and not vol[:, far][:, :, ~thin].any()
    assert not ref[:, 2, 0].any()                                     # (-40, -40): exactly 0 at level 0, for any r <= 7
    assert not ref[:, kinds == "outside", 0].any() and (kinds == "outside").sum() == 5
    if min(H, W) > 5:                                                 # (the other coordinate, 5, is inside the map)
        assert ref[:, kinds == "edge"].any(-1).all()                  # the last positions whose window still meets the map
    zero = np.where((kinds == "zero")[None, :, None], 0.0, coords)     # -0.0 and 1e-30 are 0 up to 1e-30 x a correlation
    at0 = corr_util.np_corr_lookup(fmaps, targets, np.where(nonfinite[None, :, None], calm, zero), L, r).reshape(ref.shape)
    assert np.abs(at0 - ref).max() <= 1e-28 and (kinds == "zero").sum() == 3
