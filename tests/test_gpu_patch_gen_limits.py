"""The tie rule of the patch selection, exactly, and the entry's limits: `bt_patch_generate` (csrc/patch_gen.hip) on
constructed integer-valued gradient maps of 8 x 16 for a 33 x 65 image.  There every intermediate of the score is dyadic
((W-1) = 64, (H-1) = 32, Wp-1 = 15 and Hp-1 = 7 meet only powers of two in the denominators), so torch's CPU grid_sample
gives the exact rational value and so does the kernel: the device's selection must equal `torch.argsort(stable=True)` of
the CPU scores index for index, whichever of the tied candidates that is."""
import numpy as np
import pytest
import torch

import patches_util as pu
from batrack_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, G, HP, WP = 33, 65, 2, 8, 16
WG, HG = W // G, H // G


def ux_exact(t):
    """The draw u with fl(fl(u * 0.7f) + 0.15f) == t exactly (t in [0.5, 0.85): the products there step finer than t's ulp)."""
    t = np.float32(t)
    u = np.float32((np.float64(t) - 0.15) / 0.7)
    for _ in range(16):
        u = np.nextafter(u, np.float32(0))
    for _ in range(33):
        if np.float32(np.float32(u * np.float32(0.7)) + np.float32(0.15)) == t:
            return u
        u = np.nextafter(u, np.float32(2))
    raise AssertionError(f"no draw maps to {t}")


def ux_near(px):
    """A draw that lands px pixels into its cell (not exact)."""
    return np.float32((px / WG - 0.15) / 0.7)


def make_draws(gm, seed):
    """[4, 8*gm] draws: uniform, then the first eight of every cell placed by hand (see the assertions in the test)."""
    rng = np.random.default_rng(seed)
    C = 8 * gm
    ux, uy = rng.random((G * G, C), np.float32), rng.random((G * G, C), np.float32)
    for c in range(G * G):
        cx = c % G
        ux[c, :8] = [ux_near(20.2), ux_near(19.9), ux_near(20.4), ux_exact(16.5 / WG), ux_exact(17.5 / WG), ux_near(24.3),
                     ux_near(32.0) if cx == 1 else ux_near(26.1), ux_near(24.3)]
        uy[c, 0] = 0.5                                         # 8 rows into the cell: map rows 1 and 2 in the cells of the top row
        uy[c, 2] = uy[c, 1]                                    # two places in one pixel: a tie in either rows mode
        uy[c, 7] = uy[c, 5]                                    # the same place twice
    return ux, uy


def make_map(seed, special):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 3, (HP, WP)).astype(np.float32)
    g[:, 4:8] = 2.0                                            # columns with equal values: equal scores from different columns
    g[2:5, 9:13] = 1.0
    if special:
        g[0, 3] = np.nan                                       # read by rows="reference" (map rows 0 and 1 only)
        g[1, 4] = np.nan                                       # read by rows="image" from the placed candidates at column 20
        g[1, 10] = np.inf
        g[3, 14] = np.nan
    return g


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(2)
    image = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    depth = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    return image, depth, torch.as_tensor(image, device=DEV), torch.as_tensor(depth, device=DEV)


def call(g, image, depth, ux, uy, gm, rows, Gc=G):
    M = Gc * Gc * gm
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    gd, uxd, uyd = up(g), up(ux), up(uy)
    out = dict(patches=torch.full((M, 3), -1.0, device=DEV), clr=torch.full((M, 3), -1.0, device=DEV),
               colors=torch.zeros((M, 3), dtype=torch.uint8, device=DEV), coords=torch.full((M, 2), -1.0, device=DEV),
               sel=torch.full((M,), -1, dtype=torch.int32, device=DEV))
    a = _lib.PatchArgs(g=gd.data_ptr(), Hp=HP, Wp=WP, image=image.data_ptr(), dtype=_lib.BT_IMAGE_U8,
                       rows_mode=_lib.BT_PATCH_ROWS[rows], H=H, W=W, stride_c=image.stride(0), stride_y=image.stride(1),
                       stride_x=image.stride(2), depth=depth.data_ptr(), ux=uxd.data_ptr(), uy=uyd.data_ptr(), G=Gc, gm=gm,
                       **{k: v.data_ptr() for k, v in out.items()})
    rc = _lib.lib().bt_patch_generate(a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def test_the_placed_candidates_are_where_they_should_be():
    ux, uy = make_draws(1, 0)
    xg, _ = pu.candidates(ux, uy, G, H, W)
    xg = xg.numpy()
    for c in range(G * G):
        o = (c % G) * WG
        assert np.round(xg[c, :3]).tolist() == [o + 20] * 3 and len(set(xg[c, :3].tolist())) == 3     # one column, three places
        assert xg[c, 3] == o + 16.5 and xg[c, 4] == o + 17.5                                          # exactly halfway
        assert np.rint(xg[c, 3]) == o + 16 and np.rint(xg[c, 4]) == o + 18                            # to the even column
        assert np.round(xg[c, 5]) == np.round(xg[c, 7]) == o + 24
    assert np.round(xg[1, 6]) == np.round(xg[3, 6]) == W - 1                                          # the last column


@pytest.mark.parametrize("rows", ["reference", "image"])
@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("gm", [1, 2, 8, 9, 128])               # C = 8, 16, 64 (a full wave), 72 (the first LDS size), 1024 (the last)
def test_tie_rule_exact(scene, gm, special, rows):
    image, depth, image_d, depth_d = scene
    g = make_map(gm, special)
    ux, uy = make_draws(gm, 10 + gm)
    rc, r = call(g, image_d, depth_d, ux, uy, gm, rows)
    assert rc == _lib.BT_OK
    xg, yg = pu.candidates(ux, uy, G, H, W)
    sc = pu.scores(g, xg, yg, H, W, rows)
    want = pu.select(sc, gm).numpy()
    ties = sum(int(len(np.unique(row[~np.isnan(row)])) < (~np.isnan(row)).sum()) for row in sc.numpy())
    assert ties == G * G                                         # every cell has candidates of exactly equal score
    if special:
        assert np.isnan(sc.numpy()).any()
    assert np.array_equal(r["sel"], want)
    at = pu.patch_rows(image, depth, xg, yg, want, gm)
    for k in ("patches", "clr", "colors", "coords"):
        assert r[k].tobytes() == at[k].tobytes(), k


def test_unsupported_and_invalid(scene):
    image, depth, image_d, depth_d = scene
    ux, uy = make_draws(1, 0)
    g = make_map(0, False)
    rc, r = call(g, image_d, depth_d, np.zeros((4, 8 * 129), np.float32), np.zeros((4, 8 * 129), np.float32), 129, "reference")
    assert rc == _lib.BT_EUNSUPPORTED and (r["sel"] == -1).all() and (r["patches"] == -1).all()      # nothing was launched
    rc, r = call(g, image_d, depth_d, ux, uy, 1, "reference", Gc=34)                                 # H_grid < 1
    assert rc == _lib.BT_EINVAL and (r["sel"] == -1).all()
    with pytest.raises(RuntimeError, match="patch generation"):
        _lib.check(_lib.BT_EUNSUPPORTED, "bt_patch_generate")
