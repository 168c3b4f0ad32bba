#!/usr/bin/env python3
"""Golden vectors for the first step of a frame: the reference's `BATRACK.generate_patches` (main/batrack.py:230-325, mode
`grid_grad_<G>`) and `BATRACK.init_depth(mode='dmap')` (:917-934), and through them `__image_gradient_2` (:214-221),
`altcorr.patchify` (backend/altcorr/correlation.py:51-68) and `bilinear_sample2d` (frontend/core/model_utils.py:75-158),
all UNMODIFIED, on an `object.__new__(BATRACK)` whose attributes this script fills (no __init__: it loads network
weights), where the reference checkout is at hand (BATRACK_REFERENCE, default /root/reference).  float32, CPU.

Stand-ins: tests/golden/refstubs first on sys.path (its `cuda_corr.patchify_forward` is the gather below the reference's
own Python blend) and the two empty modules `main.slam_visualizer` and `main.frontend.md_tracker`, as for the other
fixtures.  The two methods name the device "cuda" literally; this script redirects THAT NAME ONLY while they run:
`torch.rand` (which also records both draws) and `torch.ones` drop `device="cuda"`, and `torch.Tensor.to` ignores a
"cuda" argument.  `F.grid_sample` is wrapped to record what goes in (the gradient map) and what comes out (the
per-candidate scores); it computes nothing itself.

Writes tests/golden/patch_gen.npz.  Per case c:
  c.image      A: [H,W,3] uint8 (the pipeline's HWC array; c.hwc = 1), B: [3,H,W] float32, integer-valued, C: [3,H,W] uint8
  c.depth [H,W], c.G, c.M, c.hwc, c.seed
  c.ux, c.uy [G*G, 8]   the two torch.rand results of :291-292, in that order
  c.g [Hp,Wp]           the reference's gradient map;   c.scores [G*G, 8]   its score of every candidate
  c.patches0 [M,3]      generate_patches' patches (x, y, 1) at the patch centre, before init_depth
  c.patches [M,3]       after init_depth(mode='dmap');  c.clr [M,3]
Cases: A 64x96, G=4; B 48x80, G=2, whose depth has values below 1e-2 and a NaN under selected points; C 50x70 (neither
side a multiple of 4 or of G), G=3.  The seed of each case is the first for which (asserted) no cell has two scores whose
difference lies between 1e-5 and 1e-4 of the cell's largest, and at least three quarters of the cells have a single
candidate within 1e-5 of the top: what is not a tie is then far from one.
Only generated inputs and numeric outputs are written.

    python tests/golden/make_golden_patch_gen.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("BATRACK_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(HERE, "refstubs"), os.path.join(REF, "main"), REF, ROOT, os.path.join(ROOT, "tests")]
for name, attr in (("main.slam_visualizer", "LEAPVisualizer"), ("main.frontend.md_tracker", "MDTracker")):
    mod = types.ModuleType(name)
    setattr(mod, attr, type(attr, (), {}))
    sys.modules[name] = mod

import main.batrack as ref_batrack                     # noqa: E402  (reference, unmodified)

import patches_util as pu                              # noqa: E402  (only the names and the cell predicate)

torch.set_num_threads(4)
SPECS = dict(A=(64, 96, 4, "u8_hwc"), B=(48, 80, 2, "f32"), C=(50, 70, 3, "u8"))


class Settings:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Redirect:
    """While active: the literal device name "cuda" means the CPU; the draws and grid_sample's input and output are kept."""

    def __enter__(self):
        self.draws, self.maps, self.scores = [], [], []
        self.saved = (torch.rand, torch.ones, torch.Tensor.to, ref_batrack.F.grid_sample)
        rand, ones, to, grid_sample = self.saved
        drop = lambda kw: {k: v for k, v in kw.items() if not (k == "device" and str(v) == "cuda")}

        def rec_rand(*a, **kw):
            self.draws.append(rand(*a, **drop(kw)))
            return self.draws[-1].clone()

        def to_cpu(t, *a, **kw):
            a, kw = [x for x in a if str(x) != "cuda"], drop(kw)
            return to(t, *a, **kw) if a or kw else t

        def rec_sample(inp, grid, **kw):
            out = grid_sample(inp, grid, **kw)
            self.maps.append(inp.clone())
            self.scores.append(out.clone())
            return out
        torch.rand = rec_rand
        torch.ones = lambda *a, **kw: ones(*a, **drop(kw))
        torch.Tensor.to = to_cpu
        ref_batrack.F.grid_sample = rec_sample
        return self

    def __exit__(self, *exc):
        torch.rand, torch.ones, torch.Tensor.to, ref_batrack.F.grid_sample = self.saved


def make_image(rng, H, W, kind):
    """Blocks of random colour with a little noise: gradients of very different sizes from cell to cell."""
    bh, bw = rng.integers(3, 9), rng.integers(3, 9)
    blocks = rng.integers(0, 256, (3, -(-H // bh), -(-W // bw)))
    im = np.kron(blocks, np.ones((1, bh, bw), np.int64))[:, :H, :W] + rng.integers(-6, 7, (3, H, W))
    im = np.clip(im, 0, 255)
    if kind == "u8_hwc":
        return np.ascontiguousarray(im.transpose(1, 2, 0)).astype(np.uint8)
    return im.astype(np.float32 if kind == "f32" else np.uint8)


def run_case(seed, H, W, G, kind):
    rng = np.random.default_rng(seed)
    image = make_image(rng, H, W, kind)
    depth = rng.uniform(0.5, 8.0, (H, W)).astype(np.float32)
    chw = torch.from_numpy(image).permute(2, 0, 1) if kind == "u8_hwc" else torch.from_numpy(image)
    o = object.__new__(ref_batrack.BATRACK)
    o.cfg = Settings(slam=Settings(PATCH_GEN=f"grid_grad_{G}"))
    o.M, o.P, o.ht, o.wd = G * G, 1, H, W
    o.local_window = [chw]
    o.poses_ = torch.zeros(1, 7)
    torch.manual_seed(seed)
    with Redirect() as r, torch.no_grad():
        patches, clr = o.generate_patches(chw)            # the reference's method as it lies there
    assert len(r.draws) == 2 and len(r.maps) == 1
    patches0 = patches.reshape(-1, 3).numpy().copy()
    sc = r.scores[0].reshape(G * G, 8).numpy()
    if kind == "f32":                                      # case B: the depth's special values under selected points
        px, py = np.floor(patches0[:, 0]).astype(int), np.floor(patches0[:, 1]).astype(int)
        depth[py[0], px[0]] = np.nan
        depth[py[1]:py[1] + 2, px[1]:px[1] + 2] = 1e-3
        depth[py[-1]:py[-1] + 2, px[-1]:px[-1] + 2] = [[5e-3, 2e-2], [0.0, 9e-3]]   # the cell of the last row and column
    with Redirect(), torch.no_grad():
        after = o.init_depth(patches.clone(), torch.from_numpy(depth)[None], mode="dmap")
    out = dict(image=image, depth=depth, G=np.int64(G), M=np.int64(G * G), hwc=np.int64(kind == "u8_hwc"), seed=np.int64(seed),
               ux=r.draws[0].numpy(), uy=r.draws[1].numpy(), g=r.maps[0][0, 0].numpy(), scores=sc, patches0=patches0,
               patches=after.reshape(-1, 3).numpy().copy(), clr=clr.reshape(-1, 3).numpy().copy())
    return out


def conditions(sc):
    """The two conditions of the module's text on a case's scores [cells, 8]."""
    sc = sc.astype(np.float64)
    top = np.abs(sc).max(1)
    diff = np.abs(sc[:, :, None] - sc[:, None, :])
    rel = diff / np.where(top > 0, top, 1.0)[:, None, None]
    gap = not ((rel > 1e-5) & (rel < 1e-4)).any()
    single = pu.single_candidate_cells(sc).mean() >= 0.75
    return gap and single


def main():
    out = {}
    assert tuple(SPECS) == pu.CASES
    for c, (H, W, G, kind) in SPECS.items():
        for seed in range(100, 200):
            r = run_case(seed, H, W, G, kind)
            if conditions(r["scores"]):
                break
        else:
            raise SystemExit(f"case {c}: no seed meets the conditions")
        assert conditions(r["scores"])
        assert r["g"].shape == ((H + 1) // 4, (W + 1) // 4) and r["g"].dtype == np.float32
        sel = r["scores"].argmax(1)
        single = pu.single_candidate_cells(r["scores"])
        if c == "B":
            d = r["depth"]
            assert np.isnan(d).sum() == 1 and (d < 1e-2).sum() >= 4 and np.isnan(r["patches"][:, 2]).sum() == 1
            assert (r["patches"][:, 2] == 100.0).any()                  # a sample below 1e-2, clamped
            assert r["patches0"][-1, 0] >= W // G and r["patches0"][-1, 1] >= H // G   # a selected point of the last cell
        print(f"case {c}: {H}x{W} G={G} {kind} seed {int(r['seed'])}: {int(single.sum())} of {G * G} cells with a single candidate at the top, "
              f"argmax {sel.tolist()}")
        for name, v in r.items():
            out[f"{c}.{name}"] = v
    path = os.path.join(HERE, "patch_gen.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "observe_window.npz"))


if __name__ == "__main__":
    main()
