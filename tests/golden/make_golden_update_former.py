#!/usr/bin/env python3
"""Golden vectors for the update transformer: the reference's UNMODIFIED `UpdateFormer` and `AttnBlock`
(main/frontend/core/cotracker/blocks.py:388-457, :280-305) on torch-CPU, in float32 and in float64, where the reference
checkout is at hand.

Stand-ins.  `timm` is not installed: tests/golden/refstubs_timm, first on sys.path, restates the two classes the reference
imports from it (`Attention`, `Mlp`) in plain torch — an UNPINNED restatement, see its docstring.  tests/golden/refstubs
(unchanged) supplies the empty `torchvision` the same file imports; `einops` is installed.

Weights and inputs come from tests/update_former_util.make_inputs (seeded, drawn in float64, rounded to float32) and are NOT
stored: the fixture keeps their digests.  Writes tests/golden/update_former.npz; per case c of update_former_util.CASES:
  c.digest.<name>   float64 [3] of every weight, bias and of the input x
  c.out32           float32 [1, N, S, 19]   the reference's float32 run
  c.out64           float64 [1, N, S, 19]   its float64 run on the same values
  c.gate            max |out32 - out64|
and `signatures`: str(inspect.signature(UpdateFormer.forward)).  Only digests of inputs we generated and numeric results are
written.

    BATRACK_REFERENCE=<reference checkout> python tests/golden/make_golden_update_former.py
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
sys.path[:0] = [os.path.join(HERE, "refstubs_timm"), os.path.join(HERE, "refstubs"), REF, os.path.join(ROOT, "tests")]

import main.frontend.core.cotracker.blocks as blocks                         # noqa: E402  (reference, unmodified)

import update_former_util as U                                               # noqa: E402

torch.set_num_threads(4)


def run_reference(c, dtype):
    spec = U.CASES[c]
    d = U.make_inputs(**spec)
    model = blocks.UpdateFormer(space_depth=spec["space_depth"], time_depth=spec["time_depth"], input_dim=U.INPUT_DIM,
                                hidden_size=U.HIDDEN, num_heads=U.HEADS, output_dim=U.OUTPUT_DIM, mlp_ratio=U.MLP / U.HIDDEN).to(dtype).eval()
    assert isinstance(model.time_blocks[0], blocks.AttnBlock) and model.time_blocks[0].attn.head_dim == U.HEAD_DIM
    model.load_state_dict({k: torch.as_tensor(v, dtype=dtype) for k, v in d.items() if k != "x"}, strict=True)
    with torch.no_grad():
        out = model(torch.as_tensor(d["x"], dtype=dtype))
    assert out.shape == (1, spec["N"], spec["S"], U.OUTPUT_DIM) and out.dtype == dtype
    return out, d


def main():
    out = {"signatures": np.array([str(inspect.signature(blocks.UpdateFormer.forward))])}
    for c, spec in U.CASES.items():
        (o32, d), (o64, __) = run_reference(c, torch.float32), run_reference(c, torch.float64)
        for name, v in d.items():
            out[f"{c}.digest.{name}"] = U.digest(v)
        out[f"{c}.out32"], out[f"{c}.out64"] = o32.numpy(), o64.numpy()
        out[f"{c}.gate"] = np.float64((o32.double() - o64).abs().max())
        print(f"case {c} ({spec}): gate {out[f'{c}.gate']:.3e}, max |out| {float(o64.abs().max()):.3f}")
    path = os.path.join(HERE, "update_former.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
