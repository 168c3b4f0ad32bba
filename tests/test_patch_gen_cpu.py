"""Patch selection and depth initialisation of a new frame, without a GPU: the restatement of include/batrack_patches.h in
tests/patches_util.py against the fixture made from the reference's unmodified `generate_patches` and `init_depth`
(tests/golden/patch_gen.npz), the fixture's own conditions, the C entries' refusals and the configuration's."""
import ctypes

import numpy as np
import pytest

import patches_util as pu
from batrack_amd import _lib
from batrack_amd.frontend.patches import PatchGenConfig


@pytest.fixture(scope="module")
def golden():
    return np.load(pu.GOLDEN)


@pytest.fixture(scope="module")
def restated(golden):
    out = {}
    for c in pu.CASES:
        d = pu.load_case(c, golden)
        out[c] = (d, pu.restate(pu.image_chw(d), d["depth"], d["ux"], d["uy"], int(d["G"]), 1))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", pu.CASES)
def test_restatement_reproduces_the_fixture(restated, case):
    d, r = restated[case]
    one = pu.single_candidate_cells(d["scores"])
    assert one.any()
    assert pu.admissible(d["scores"], r["sel"], 1)
    assert pu.admissible(d["scores"], d["scores"].argmax(1), 1)              # the reference's own choice
    # where the choice is forced, every number is the reference's, bit for bit
    assert np.array_equal(r["sel"][one], d["scores"].argmax(1)[one])
    assert same_bits(r["patches"][one], d["patches"][one])
    assert same_bits(r["patches"][one][:, :2], d["patches0"][one][:, :2])
    assert same_bits(r["clr"][one], d["clr"][one])
    # everywhere: the rows at the reference's selection are the reference's rows (the elementwise part has no freedom)
    at = pu.patch_rows(pu.image_chw(d), d["depth"], r["xg"], r["yg"], _reference_sel(d, r), 1)
    assert same_bits(at["patches"], d["patches"]) and same_bits(at["clr"], d["clr"])


def _reference_sel(d, r):
    """Which candidate the reference took in every cell, read off its unrounded coordinates: the patch's x is the blend
    of the coordinate grid at the candidate, so the candidate is the one whose rows reproduce it."""
    G2 = d["scores"].shape[0]
    sel = np.zeros(G2, np.int64)
    img, dep = pu.image_chw(d), d["depth"]
    for i in range(8):
        rows = pu.patch_rows(img, dep, r["xg"], r["yg"], np.full(G2, i), 1)
        hit = (rows["patches"][:, :2].view(np.uint32) == d["patches0"][:, :2].view(np.uint32)).all(1)
        sel[hit] = i
    return sel


@pytest.mark.parametrize("case", pu.CASES)
def test_restated_map_within_the_derived_bound(restated, case):
    d, r = restated[case]
    assert r["g"].shape == d["g"].shape and r["g"].dtype == np.float32
    err = np.abs(r["g"].astype(np.float64) - d["g"]) / np.abs(d["g"])
    print(f"case {case}: largest relative difference of the restated map from the reference's {err.max():.3e}, "
          f"{int((r['g'] != d['g']).sum())} of {d['g'].size} values differ")
    assert (d["g"] > 0).all() and err.max() <= pu.G_RTOL
    # the reference's scores are its grid_sample of its own map: the restatement's scores on that map are the same numbers
    xg, yg = pu.candidates(d["ux"], d["uy"], int(d["G"]), *d["depth"].shape)
    assert same_bits(pu.scores(d["g"], xg, yg, *d["depth"].shape).numpy(), d["scores"])


@pytest.mark.parametrize("case", pu.CASES)
def test_fixture_conditions(golden, case):
    d = pu.load_case(case, golden)
    sc = d["scores"].astype(np.float64)
    rel = np.abs(sc[:, :, None] - sc[:, None, :]) / np.abs(sc).max(1)[:, None, None]
    assert not ((rel > 1e-5) & (rel < 1e-4)).any()
    assert pu.single_candidate_cells(sc).mean() >= 0.75
    H, W = d["depth"].shape
    assert pu.image_chw(d).shape == (3, H, W) and d["ux"].shape == d["uy"].shape == (int(d["G"]) ** 2, 8)
    if case == "A":
        assert d["image"].dtype == np.uint8 and d["image"].shape == (64, 96, 3)
    if case == "B":
        assert d["image"].dtype == np.float32 and np.array_equal(d["image"], np.round(d["image"]))
        assert np.isnan(d["depth"]).sum() == 1 and (d["depth"] < 1e-2).any()
        assert np.isnan(d["patches"][:, 2]).sum() == 1 and (d["patches"][:, 2] == 100.0).any()
    if case == "C":
        assert H % 4 and W % 4 and H % int(d["G"]) and W % int(d["G"])


def test_more_than_one_patch_a_cell_restated():
    """gm > 1 (the reference raises there): per cell the top gm in ascending rank, distinct, at c*gm + r."""
    rng = np.random.default_rng(5)
    sc = rng.integers(0, 4, (9, 16)).astype(np.float32)
    sc[0, 3] = np.nan
    sel = pu.select(sc, 2).numpy().reshape(9, 2)
    assert sel[0, 1] == 3
    for c in range(9):
        order = sorted(range(16), key=lambda i: (np.isnan(sc[c, i]), sc[c, i] if not np.isnan(sc[c, i]) else 0.0, i))
        assert sel[c].tolist() == order[-2:]
    assert pu.admissible(np.nan_to_num(sc, nan=9.0), sel.reshape(-1), 2)
    assert not pu.admissible(np.nan_to_num(sc, nan=9.0), np.repeat(sel[:, 1], 2), 2)         # a candidate taken twice


def test_argument_errors_return_codes():
    """Every check returns before anything is enqueued: the pointers below are never dereferenced (no GPU here)."""
    L = _lib.lib()
    EINVAL, EUNS = _lib.BT_EINVAL, _lib.BT_EUNSUPPORTED
    p = lambda i: 0x10000 * i
    grad = lambda image=p(1), dtype=0, H=64, W=96, g=p(2): L.bt_image_gradient(image, dtype, H, W, 1, 3 * W, 3, g, None)
    assert grad(image=None) == EINVAL and grad(g=None) == EINVAL and grad(dtype=2) == EINVAL
    assert grad(H=2) == EINVAL and grad(W=2) == EINVAL and grad(H=32769) == EUNS and grad(W=32769) == EUNS

    def gen(**kw):
        v = dict(g=p(1), Hp=16, Wp=24, image=p(2), dtype=0, rows_mode=0, H=64, W=96, stride_c=1, stride_y=288, stride_x=3,
                 depth=p(3), ux=p(4), uy=p(5), G=4, gm=1, patches=p(6), clr=p(7), colors=p(8), coords=p(9), sel=p(10))
        v.update(kw)
        return L.bt_patch_generate(_lib.PatchArgs(**v), None)
    assert L.bt_patch_generate(None, None) == EINVAL
    for name in ("g", "image", "depth", "ux", "uy", "patches"):
        assert gen(**{name: None}) == EINVAL, name
    assert gen(H=2, Hp=0) == EINVAL and gen(W=2, Wp=0) == EINVAL and gen(G=0) == EINVAL and gen(gm=0) == EINVAL
    assert gen(G=65) == EINVAL and gen(G=97) == EINVAL                      # H_grid < 1, W_grid < 1
    assert gen(dtype=2) == EINVAL and gen(rows_mode=2) == EINVAL and gen(Hp=15) == EINVAL and gen(Wp=25) == EINVAL
    assert gen(gm=129) == EUNS and gen(H=32769, Hp=8192) == EUNS and gen(W=32769, Wp=8192) == EUNS
    assert "patch generation" in _lib.ERRORS[EUNS] and "1024 candidates" in _lib.ERRORS[EUNS]


def test_sources_and_symbols():
    assert "patch_gen.hip" in _lib.SOURCES and "sample_taps.hpp" in _lib.HEADERS
    assert any(h.endswith("batrack_patches.h") for h in _lib.HEADERS)
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "bt_image_gradient") and hasattr(L, "bt_patch_generate")
    assert ctypes.sizeof(_lib.PatchArgs) == 20 * 8


def test_configuration():
    assert PatchGenConfig().grid() == (20, 1)
    assert PatchGenConfig("grid_grad_4", 32).grid() == (4, 2)
    for mode in ("uniform", "random", "sift", "grid_grad", "grid_grad_x", "grid_grad_0", "grid_20"):
        with pytest.raises(ValueError, match=mode):
            PatchGenConfig(PATCH_GEN=mode).grid()
    with pytest.raises(ValueError, match="multiple"):
        PatchGenConfig("grid_grad_4", 20).grid()
    with pytest.raises(ValueError, match="rows"):
        PatchGenConfig(rows="both").grid()
