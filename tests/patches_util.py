"""Test-side helpers for the patch selection of a new frame (tests/golden/patch_gen.npz, made by
tests/golden/make_golden_patch_gen.py): the fixture's names, a numpy statement of (a) and a torch-CPU statement of
(b)-(d) of include/batrack_patches.h, for any patches-per-cell and either rows mode, and the admissibility check of a
selection.  Test infrastructure only."""
import os

import numpy as np
import torch
import torch.nn.functional as F

CASES = ("A", "B", "C")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_gen.npz")
# restated g against the reference's CPU map: each of the 16 positive terms is off by at most one ulp of a root that is
# not correctly rounded there (2^-23 relative), plus at most 16 accumulation roundings of 2^-24 and the final one:
# 9.5 * 2^-23 = 1.13e-6
G_RTOL = 1.2e-6


def load_case(c, z=None):
    z = z if z is not None else np.load(GOLDEN)
    return {k[len(c) + 1:]: z[k] for k in z.files if k.startswith(c + ".")}


def image_chw(d):
    """The case's image as the [3, H, W] numpy view the pipeline hands over (HWC storage is permuted, not copied)."""
    im = d["image"]
    return im.transpose(2, 0, 1) if int(d["hwc"]) else im


def grad_map_np(image):
    """(a): image [3, H, W] uint8 or integer-valued float32 -> g [Hp, Wp] float32, IEEE root, the 16 terms added row-major."""
    s = image.astype(np.int64).sum(0) if image.dtype == np.uint8 else (image[0] + image[1]) + image[2]
    H, W = s.shape
    p = np.zeros((H + 2, W + 2), s.dtype)
    p[1:-1, 1:-1] = s
    dx = p[:-1, 1:] - p[:-1, :-1]
    dy = p[1:, :-1] - p[:-1, :-1]
    q = dx * dx + dy * dy
    v = np.sqrt(q.astype(np.float32))
    Hp, Wp = (H + 1) // 4, (W + 1) // 4
    acc = np.zeros((Hp, Wp), np.float32)
    for a in range(4):
        for b in range(4):
            acc = acc + v[a:4 * Hp:4, b:4 * Wp:4]
    return acc * np.float32(0.0625)


def candidates(ux, uy, G, H, W):
    """(b), first half: draws [G*G, C] -> (xg, yg) [G*G, C] float32, every operation rounded."""
    ux, uy = torch.as_tensor(ux), torch.as_tensor(uy)
    Wg, Hg = W // G, H // G
    cell = torch.arange(G * G, device=ux.device)
    ox = ((cell % G) * Wg).float()[:, None]
    oy = ((cell // G) * Hg).float()[:, None]
    x = ux * (1 - 2 * 0.15) + 0.15                       # batrack.py:291-292: the scalars become 0.7f and 0.15f
    y = uy * (1 - 2 * 0.15) + 0.15
    return x * float(Wg) + ox, y * float(Hg) + oy


def scores(g, xg, yg, H, W, rows="reference"):
    """(b), second half: the score of every candidate by torch's own grid_sample on the CPU.  g [Hp, Wp]."""
    xn = torch.round(xg) / (W - 1) * 2.0 - 1.0
    yn = (xn if rows == "reference" else torch.round(yg)) / (H - 1) * 2.0 - 1.0
    grid = torch.stack([xn, yn], -1).reshape(1, 1, -1, 2)
    gg = F.grid_sample(torch.as_tensor(g)[None, None], grid, mode="bilinear", align_corners=True)
    return gg.reshape(xg.shape)


def select(sc, gm):
    """(c): [G*G, C] scores -> sel [G*G*gm] int64, ascending by (score, index), NaN highest, the top gm in ascending rank."""
    return torch.argsort(torch.as_tensor(sc), dim=-1, stable=True)[:, -gm:].reshape(-1)


def _blend(planes, x, y):
    """correlation.py:55-66 at radius 0: planes [K, H, W] float32, zeros outside; x, y [M] -> [M, K]."""
    K, H, W = planes.shape
    fx, fy = torch.floor(x), torch.floor(y)
    j, i = fx.long(), fy.long()
    dx, dy = (x - fx)[:, None], (y - fy)[:, None]

    def tap(ii, jj):
        ok = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
        v = planes[:, ii.clamp(0, H - 1), jj.clamp(0, W - 1)].T
        return torch.where(ok[:, None], v, torch.zeros_like(v))
    x00 = (1 - dy) * (1 - dx) * tap(i, j)
    x01 = (1 - dy) * dx * tap(i, j + 1)
    x10 = dy * (1 - dx) * tap(i + 1, j)
    x11 = dy * dx * tap(i + 1, j + 1)
    return x00 + x01 + x10 + x11


def _bilinear_sample2d(im, x, y):
    """model_utils.py:75-158 on one [H, W] map."""
    H, W = im.shape
    x0, y0 = torch.floor(x).int(), torch.floor(y).int()
    x1, y1 = x0 + 1, y0 + 1
    cx0, cx1, cy0, cy1 = x0.clamp(0, W - 1).long(), x1.clamp(0, W - 1).long(), y0.clamp(0, H - 1).long(), y1.clamp(0, H - 1).long()
    w00 = (x1.float() - x) * (y1.float() - y)
    w01 = (x - x0.float()) * (y1.float() - y)
    w10 = (x1.float() - x) * (y - y0.float())
    w11 = (x - x0.float()) * (y - y0.float())
    return w00 * im[cy0, cx0] + w01 * im[cy0, cx1] + w10 * im[cy1, cx0] + w11 * im[cy1, cx1]


def patch_rows_t(img, depth, xg, yg, sel, gm):
    """(d) at a given selection, tensors in and out (any device): img [3, H, W] float32, depth [H, W], xg / yg [G*G, C],
    sel [G*G*gm] -> patches [M, 3], clr [M, 3], colors [M, 3] uint8, coords [M, 2]."""
    sel = sel.long().reshape(-1, gm)
    cx, cy = torch.gather(xg, 1, sel).reshape(-1), torch.gather(yg, 1, sel).reshape(-1)
    _, H, W = img.shape
    ar = lambda n: torch.arange(n, device=img.device).float()
    grid = torch.stack([ar(W)[None, :].expand(H, W), ar(H)[:, None].expand(H, W)])
    pxy = _blend(grid, cx, cy)
    clr = _blend(img, cx + 0.5, cy + 0.5)
    d = _bilinear_sample2d(depth, pxy[:, 0], pxy[:, 1])
    disp = 1.0 / d.clamp(min=1e-2)
    return torch.cat([pxy, disp[:, None]], 1), clr, clr.to(torch.uint8), torch.stack([cx, cy], 1)


def patch_rows(image, depth, xg, yg, sel, gm):
    """patch_rows_t on the CPU from numpy: image [3, H, W] uint8 or float32 -> dict of numpy arrays."""
    img = torch.as_tensor(np.ascontiguousarray(image)).float()
    out = patch_rows_t(img, torch.as_tensor(depth), xg, yg, torch.as_tensor(np.asarray(sel)), gm)
    return dict(zip(("patches", "clr", "colors", "coords"), (t.numpy() for t in out)))


def restate(image, depth, ux, uy, G, gm, rows="reference", g=None):
    """(a)-(d) on the CPU: dict with g, xg, yg, scores, sel and the rows of patch_rows."""
    _, H, W = image.shape
    g = grad_map_np(image) if g is None else g
    xg, yg = candidates(ux, uy, G, H, W)
    sc = scores(g, xg, yg, H, W, rows)
    sel = select(sc, gm)
    out = patch_rows(image, depth, xg, yg, sel, gm)
    out.update(g=g, xg=xg, yg=yg, scores=sc.numpy(), sel=sel.numpy())
    return out


def single_candidate_cells(sc, band=1e-5):
    """Cells [G*G] bool whose top score has no other candidate within band * max|score| of it."""
    sc = np.asarray(sc, np.float64)
    top = sc.max(1, keepdims=True)
    return ((top - sc) <= band * np.abs(sc).max(1, keepdims=True)).sum(1) == 1


def admissible(sc, sel, gm, band=1e-5):
    """The selected indices of a cell are distinct, and slot r's reference score is within band * max|score| of the
    reference's (C - gm + r)-th sorted score.  sc [G*G, C] reference scores, sel [G*G*gm]."""
    sc = np.asarray(sc, np.float64)
    sel = np.asarray(sel).astype(np.int64).reshape(-1, gm)
    C = sc.shape[1]
    if sel.min() < 0 or sel.max() >= C or any(len(set(r)) != gm for r in sel.tolist()):
        return False
    want = np.sort(sc, 1)[:, C - gm:]
    got = np.take_along_axis(sc, sel, 1)
    return bool((np.abs(got - want) <= band * np.abs(sc).max(1, keepdims=True)).all())
