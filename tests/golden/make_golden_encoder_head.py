#!/usr/bin/env python3
"""Golden vectors for the encoder's head: the reference's UNMODIFIED `BasicEncoder.forward`
(main/frontend/core/cotracker/blocks.py:210-277) on torch-CPU, in float32 and in float64, where the reference checkout is at
hand.  tests/golden/refstubs first on sys.path supplies the modules the reference's file imports and this path never calls.

The encoder is built as the model builds it, `BasicEncoder(input_dim=3, output_dim=128, norm_fn="instance", stride=s)`, and
the class's own `forward` is called.  Stand-ins, assigned to that INSTANCE only:
  conv1, norm1, relu1   identities;
  layer1 .. layer4      modules that return the case's seeded maps, whatever they are given (encoder_head_util.Returns);
  conv2, conv3          the instance's own modules, their weights and (non-zero) biases re-seeded.
So everything after `layer4` — the four resizes, the concatenation, conv2, norm2, relu2, conv3 — is the reference's.

Inputs come from encoder_head_util.make_inputs (seeded, drawn in float64, rounded to float32) and are NOT stored: the fixture
keeps their digests.  Writes tests/golden/encoder_head.npz; per case c of encoder_head_util.CASES:
  c.digest.<name>   float64 [3] of the four maps, the two weights and the two biases
  c.out32           float32 [F, 128, h, w]   the reference's float32 run
  c.out64           float64: every 8th element of its float64 run on the same values
  c.gate            max |out32 - out64| over all elements
and `signature`: str(inspect.signature(BasicEncoder.forward)).  Only digests of inputs we generated and numeric results are
written.

The generator asserts that every (frame, channel) variance of conv2's output is at least 1e-3 of the case's mean variance: a
near-constant channel would turn the gate into a statement about 1 / sqrt(var + eps).  A condition on the inputs, not a
tolerance.

    BATRACK_REFERENCE=<reference checkout> python tests/golden/make_golden_encoder_head.py
"""
import inspect
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

import encoder_head_util as U                                                # noqa: E402

torch.set_num_threads(4)


def run_reference(c, dtype):
    spec = U.CASES[c]
    t = U.case_tensors(c, dtype)
    enc = blocks.BasicEncoder(input_dim=3, output_dim=128, norm_fn="instance", stride=spec["stride"]).to(dtype).eval()
    assert not enc.shallow and enc.dropout is None and isinstance(enc.norm2, torch.nn.InstanceNorm2d)
    assert not enc.norm2.affine and not enc.norm2.track_running_stats and enc.norm2.eps == 1e-5
    with torch.no_grad():
        enc.conv2.weight.copy_(t["w2"]); enc.conv2.bias.copy_(t["b2"]); enc.conv3.weight.copy_(t["w3"]); enc.conv3.bias.copy_(t["b3"])
    enc.conv1, enc.norm1, enc.relu1 = torch.nn.Identity(), torch.nn.Identity(), torch.nn.Identity()
    for name, layer in zip(U.NAMES, ("layer1", "layer2", "layer3", "layer4")):
        setattr(enc, layer, U.Returns(t[name]))
    h, w = spec["size"]
    x = torch.zeros(spec["F"], 3, h * spec["stride"], w * spec["stride"], dtype=dtype)
    with torch.no_grad():
        out = blocks.BasicEncoder.forward(enc, x)
    assert out.shape == (spec["F"], U.COUT, h, w) and out.dtype == dtype
    return out, t


def main():
    out = {"signature": np.array(str(inspect.signature(blocks.BasicEncoder.forward)))}
    for c, spec in U.CASES.items():
        (o32, __), (o64, t64) = run_reference(c, torch.float32), run_reference(c, torch.float64)
        d = U.make_inputs(**spec)
        for name in U.INPUTS:
            out[f"{c}.digest.{name}"] = U.digest(d[name])
        var = U.conv2_output(*(t64[n] for n in U.NAMES), t64["w2"], t64["b2"], spec["size"]).var(dim=(2, 3), unbiased=False)
        assert float(var.min()) >= 1e-3 * float(var.mean()), (c, float(var.min()), float(var.mean()))
        out[f"{c}.out32"] = o32.numpy()
        out[f"{c}.out64"] = o64.numpy().ravel()[::U.F64_STEP]
        out[f"{c}.gate"] = np.float64((o32.double() - o64).abs().max())
        print(f"case {c} ({spec}): gate {out[f'{c}.gate']:.3e}, max |out| {float(o64.abs().max()):.3f}, "
              f"conv2 variance min {float(var.min()):.3e} mean {float(var.mean()):.3e}")
    path = os.path.join(HERE, "encoder_head.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
