#!/usr/bin/env python3
"""Golden vectors for the position embedding at far coordinates: the reference's UNMODIFIED `sample_pos_embed`
(main/frontend/md_tracker.py:49-61, which calls bilinear_sample2d of frontend/core/model_utils.py:75-158) on torch-CPU, where
the reference checkout is at hand, at every (x, y) pair of a list of finite float32 coordinates: in-range values, values just
outside the map, and values around and far beyond 2^24 and 2^31, up to FLT_MAX.

The reference converts floor(x) to int32, which is defined only below 2^31: what it returns beyond is what the host's
conversion gives (x86: INT_MIN for every out-of-range value), and where its weights overflow it returns NaN.  The fixture
records the result as it is, NaN included; the tests compare where it is finite.

tests/golden/refstubs first on sys.path supplies the empty modules the tracker module imports and this path never calls.

Writes tests/golden/pos_embed_far.npz:
  H, W, E     the map and the embedding width (small, to keep the file to a few KB)
  values      float32 [V]        the coordinate list
  xy          float32 [V*V, 2]   every pair, x outer
  out         float32 [V*V, E]   what sample_pos_embed returned, transposed
Only coordinates we chose and numeric results are written.

    BATRACK_REFERENCE=<reference checkout> python tests/golden/make_golden_pos_embed_far.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("BATRACK_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REF:
    sys.exit("set BATRACK_REFERENCE (or pass as the first argument) to the reference checkout")
sys.path[:0] = [os.path.join(HERE, "refstubs"), REF, os.path.join(ROOT, "tests")]

import main.frontend.md_tracker as md                                        # noqa: E402  (reference, unmodified)

import track_iter_util as U                                                  # noqa: E402

torch.set_num_threads(1)


def main():
    H, W, E = U.FAR_H, U.FAR_W, U.FAR_E
    values = U.far_values(W)
    xy = U.far_pairs(values)
    with torch.no_grad():
        out = md.sample_pos_embed((H, W), E, xy[None, None])[0].t().contiguous()        # [V*V, E]
    assert out.shape == (xy.shape[0], E) and out.dtype == torch.float32
    finite = torch.isfinite(out).all(1)
    print(f"{xy.shape[0]} pairs, {int((~finite).sum())} with a non-finite row; max |finite value| {float(out[finite].abs().max()):.3f}")
    path = os.path.join(HERE, "pos_embed_far.npz")
    np.savez_compressed(path, H=np.int64(H), W=np.int64(W), E=np.int64(E), values=values.numpy(), xy=xy.numpy(), out=out.numpy())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
