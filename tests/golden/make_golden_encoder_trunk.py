#!/usr/bin/env python3
"""Golden vectors for the encoder's trunk: `layer1..layer4` of the reference's UNMODIFIED `BasicEncoder(norm_fn="instance")`
(main/frontend/core/cotracker/blocks.py:16-75 and 202-208) on torch-CPU, in float32 and in float64, where the reference
checkout is at hand.  tests/golden/refstubs first on sys.path supplies the modules the reference's file imports and this path
never calls.

The encoder is built as the model builds it and its eight `ResidualBlock`s are called as they are; only their convolutions'
weights and (non-zero) biases are re-seeded (encoder_trunk_util.make_inputs: drawn in float64, rounded to float32).  Inputs are
NOT stored: the fixture keeps their digests.  Writes tests/golden/encoder_trunk.npz; per case c of encoder_trunk_util.CASES and
level l in a, b, c, d (the outputs of layer1..4), with s = encoder_trunk_util.STEP[l]:
  c.digest.<name>     float64 [3] of `x`, of the three single-layer inputs and of every weight and bias
  c.l.out32           float32: every s-th element of the float32 run of layer1..4 on `x`
  c.l.out64           float64: every s-th element of the float64 run on the same values
  c.l.gate            max |out32 - out64| over ALL elements
  c.l.layer64         float64: every s-th element of the float64 run of that layer ALONE on its seeded input (`x` for
                      layer1, `in.layerK` otherwise)
  c.l.layer_gate      max |float32 run - float64 run| of that layer alone on that input, over all elements
(Whole maps do not fit: float64 noise does not compress, and the four levels of the three cases, twice, are 1.5 MB.  The
steps are coprime to every row length, so the samples sweep rows, columns, channels and frames.  For the same reason a
layer's own input is a seeded draw of its shape and not the float32 run's previous level, which a test could not rebuild
bit for bit on another host.)

The generator asserts two conditions on the inputs, not tolerances: every normalised map has at least 12 pixels (a 1 x 2
map's normalisation is +-1 whatever the values, and the reference's own float32 error jumps there), and every
(frame, channel) variance of every normalised map is at least 1e-3 of its map's mean variance.

    BATRACK_REFERENCE=<reference checkout> python tests/golden/make_golden_encoder_trunk.py
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

import encoder_trunk_util as U                                               # noqa: E402

torch.set_num_threads(4)


def reference_layers(t, dtype):
    enc = blocks.BasicEncoder(input_dim=3, output_dim=128, norm_fn="instance", stride=4).to(dtype).eval()
    layers = [getattr(enc, name) for name in U.LAYERS]
    with torch.no_grad():
        for name, seq in zip(U.LAYERS, layers):
            assert len(seq) == 2 and all(isinstance(b, blocks.ResidualBlock) for b in seq)
            keys = [k for k, __ in seq.named_parameters()]
            assert sorted(f"{name}.{k}" for k in keys) == sorted(n for n in U.weight_names() if n.startswith(name + "."))
            for k, p in seq.named_parameters():
                p.copy_(t[f"{name}.{k}"])
    return layers


def main():
    out = {}
    for c, spec in U.CASES.items():
        d = U.make_inputs(**spec)
        for name, v in d.items():
            out[f"{c}.digest.{name}"] = U.digest(v)
        runs = {}
        for dtype in (torch.float32, torch.float64):
            t = U.case_tensors(c, dtype)
            layers = reference_layers(t, dtype)
            with torch.no_grad():
                x, whole, alone = t["x"], [], []
                for name, seq in zip(U.LAYERS, layers):
                    x = seq(x)
                    whole.append(x)
                    alone.append(seq(U.layer_input(t, name)))
            runs[dtype] = (whole, alone)
        t64 = U.case_tensors(c, torch.float64)
        x = t64["x"]
        for name in U.LAYERS:
            assert U.conditions_hold(U.raw_maps(x, t64, name)), (c, name, "the whole run")
            assert U.conditions_hold(U.raw_maps(U.layer_input(t64, name), t64, name)), (c, name, "the layer alone")
            x = U.layer(x, t64, name)
        for i, l in enumerate(U.LEVELS):
            s = U.STEP[l]
            w32, w64, a32, a64 = runs[torch.float32][0][i], runs[torch.float64][0][i], runs[torch.float32][1][i], runs[torch.float64][1][i]
            assert tuple(w32.shape[2:]) == U.level_sizes(spec["size"])[i] and w32.dtype == torch.float32 and w64.dtype == torch.float64
            out[f"{c}.{l}.out32"] = w32.numpy().ravel()[::s]
            out[f"{c}.{l}.out64"] = w64.numpy().ravel()[::s]
            out[f"{c}.{l}.gate"] = np.float64((w32.double() - w64).abs().max())
            out[f"{c}.{l}.layer64"] = a64.numpy().ravel()[::s]
            out[f"{c}.{l}.layer_gate"] = np.float64((a32.double() - a64).abs().max())
            print(f"case {c} level {l} {tuple(w32.shape)}: gate {out[f'{c}.{l}.gate']:.3e}, alone {out[f'{c}.{l}.layer_gate']:.3e}, "
                  f"max |out| {float(w64.abs().max()):.3f}")
    path = os.path.join(HERE, "encoder_trunk.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
