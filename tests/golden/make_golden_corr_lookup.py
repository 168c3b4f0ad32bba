#!/usr/bin/env python3
"""Golden vectors for the tracker's correlation lookup: the reference's UNMODIFIED `CorrBlock`
(main/frontend/core/cotracker/blocks.py:326-385) — constructor, `corr(targets)`, `sample(coords)` — on torch-CPU, where
the reference checkout is at hand.

Stand-ins: tests/golden/refstubs first on sys.path supplies empty `timm.models.vision_transformer` (the names Attention,
Mlp) and `torchvision.transforms`, which blocks.py imports and this path never calls; `einops` is installed.

Inputs come from tests/corr_util.make_inputs (seeded, rounded to float32) and are NOT stored: the fixture keeps their
digests, so that a generator that drifts is noticed.  The coordinates are handed over as the `[..., :2]` view of a
three-column tensor, as the tracker does.  Writes tests/golden/corr_lookup.npz; per case c of corr_util.CASES:
  c.spec  [seed, S, C, H, W, N, L, r]              c.digest.fmaps / .targets / .coords3   float64 [3] each
  c.ref   [S, N, L*(2r+1)^2] float32               the reference's run on float64 inputs, as sample() returns it
  gate.c  max |float32 run - c.ref| over all entries (the reference's own float32 error on these inputs)
and `signatures`: the strings of inspect.signature for CorrBlock.__init__, corr, sample.
Only digests of inputs we generated and numeric results are written.

    python tests/golden/make_golden_corr_lookup.py
"""
import inspect
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path[:0] = [os.path.join(HERE, "refstubs"), REF, os.path.join(ROOT, "tests")]

from main.frontend.core.cotracker.blocks import CorrBlock as RefCorrBlock    # noqa: E402  (reference, unmodified)

import corr_util                                                             # noqa: E402

torch.set_num_threads(4)


def run_reference(fmaps, targets, coords3, L, r, dtype):
    t = lambda a: torch.as_tensor(a, dtype=dtype)
    with torch.no_grad():
        blk = RefCorrBlock(t(fmaps), num_levels=L, radius=r)
        blk.corr(t(targets))
        out = blk.sample(t(coords3)[..., :2])
    assert out.dtype == torch.float32 and out.is_contiguous()
    return out[0].numpy()


def main():
    out = {"signatures": np.array([str(inspect.signature(f)) for f in (RefCorrBlock.__init__, RefCorrBlock.corr, RefCorrBlock.sample)])}
    for c, spec in corr_util.CASES.items():
        fmaps, targets, coords3 = corr_util.make_inputs(**spec)
        ref64 = run_reference(fmaps, targets, coords3, spec["L"], spec["r"], torch.float64)
        ref32 = run_reference(fmaps, targets, coords3, spec["L"], spec["r"], torch.float32)
        out[f"{c}.spec"] = np.array([spec[k] for k in ("seed", "S", "C", "H", "W", "N", "L", "r")], np.int64)
        for name, a in (("fmaps", fmaps), ("targets", targets), ("coords3", coords3)):
            out[f"{c}.digest.{name}"] = corr_util.digest(a)
        out[f"{c}.ref"] = ref64
        out[f"gate.{c}"] = np.float64(np.abs(ref32.astype(np.float64) - ref64.astype(np.float64)).max())
        spec64 = corr_util.np_corr_lookup(fmaps[0], targets[0], coords3[0, ..., :2], spec["L"], spec["r"])
        spec32 = corr_util.np_corr_lookup(fmaps[0], targets[0], coords3[0, ..., :2], spec["L"], spec["r"], np.float32)
        print(f"case {c}: {ref64.shape}, max |ref| {np.abs(ref64).max():.2f}, exact zeros {int((ref64 == 0).sum())}, "
              f"gate (reference float32 vs its float64 run) {out[f'gate.{c}']:.2e}, "
              f"specification float64 vs ref {np.abs(spec64 - ref64).max():.2e}, its float32 run {np.abs(spec32 - ref64).max():.2e}")
    path = os.path.join(HERE, "corr_lookup.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
