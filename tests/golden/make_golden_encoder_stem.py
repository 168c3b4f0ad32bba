#!/usr/bin/env python3
"""Golden vectors for the encoder's stem: `relu1(norm1(conv1(x)))` of the reference's UNMODIFIED
`BasicEncoder(norm_fn="instance")` (main/frontend/core/cotracker/blocks.py:133-165 and 213-215) on torch-CPU, in float32 and in
float64, where the reference checkout is at hand.  tests/golden/refstubs first on sys.path supplies the modules the
reference's file imports and this path never calls.

The encoder is built as the model builds it and its `conv1`, `norm1`, `relu1` are called as they are; only the convolution's
weight and (non-zero) bias are re-seeded (encoder_stem_util.make_inputs: drawn in float64, rounded to float32).  Inputs are NOT
stored: the fixture keeps their digests.  Writes tests/golden/encoder_stem.npz; per case c of encoder_stem_util.CASES, with
s = encoder_stem_util.STEP[c]:
  c.digest.<name>     float64 [3] of `x`, `w` and `b`
  c.out32             float32: every s-th element of the float32 run
  c.out64             float64: every s-th element of the float64 run on the same values
  c.gate              max |out32 - out64| over ALL elements
(The steps are coprime to the row lengths, so the samples sweep rows, columns, channels and frames.)

The generator asserts two conditions on the inputs, not tolerances: the normalised map has at least 12 pixels, and every
(frame, channel) variance of it is at least 1e-3 of the map's mean variance.

    BATRACK_REFERENCE=<reference checkout> python tests/golden/make_golden_encoder_stem.py
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

import main.frontend.core.cotracker.blocks as blocks                         # noqa: E402  (reference, unmodified)

import encoder_stem_util as U                                                # noqa: E402

torch.set_num_threads(4)


def reference_stem(t, dtype):
    enc = blocks.BasicEncoder(input_dim=3, output_dim=128, norm_fn="instance", stride=4).to(dtype).eval()
    assert isinstance(enc.conv1, torch.nn.Conv2d) and isinstance(enc.norm1, torch.nn.InstanceNorm2d) and isinstance(enc.relu1, torch.nn.ReLU)
    assert tuple(enc.conv1.weight.shape) == (U.CSTEM, U.CIMG, 7, 7) and enc.conv1.bias is not None
    with torch.no_grad():
        enc.conv1.weight.copy_(t["w"])
        enc.conv1.bias.copy_(t["b"])
        return enc.relu1(enc.norm1(enc.conv1(t["x"].clone())))


def main():
    out = {}
    for c, spec in U.CASES.items():
        d = U.make_inputs(**spec)
        for name, v in d.items():
            out[f"{c}.digest.{name}"] = U.digest(v)
        t32, t64 = U.case_tensors(c, torch.float32), U.case_tensors(c, torch.float64)
        o32, o64 = reference_stem(t32, torch.float32), reference_stem(t64, torch.float64)
        raw64 = U.raw(t64["x"], t64["w"], t64["b"])
        var = raw64.var(dim=(2, 3), unbiased=False)
        assert U.conditions_hold([raw64]), c
        assert tuple(o32.shape) == (spec["F"], U.CSTEM, *U.out_size(spec["size"])) and o32.dtype == torch.float32 and o64.dtype == torch.float64
        s = U.STEP[c]
        assert np.gcd(s, o32.shape[3]) == 1
        out[f"{c}.out32"] = o32.numpy().ravel()[::s]
        out[f"{c}.out64"] = o64.numpy().ravel()[::s]
        out[f"{c}.gate"] = np.float64((o32.double() - o64).abs().max())
        print(f"case {c} {tuple(o32.shape)}: gate {out[f'{c}.gate']:.3e}, max |out| {float(o64.abs().max()):.3f}, "
              f"min variance ratio {float(var.min() / var.mean()):.3f}")
    path = os.path.join(HERE, "encoder_stem.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
