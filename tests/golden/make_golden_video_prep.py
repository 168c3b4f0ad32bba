#!/usr/bin/env python3
"""Golden vectors for the tracker's input preparation: the reference's UNMODIFIED `BATRACK._compute_sparse_tracks`
(main/batrack.py:529-587) on torch-CPU, where the reference checkout is at hand.  The method is called unbound on a plain
object (tests/video_util.StandIn) that carries the attributes it reads, once in float32 and once in float64.

Stand-ins.  tests/golden/refstubs first on sys.path and the two empty modules `main.slam_visualizer` and
`main.frontend.md_tracker` supply what the reference imports and this path never calls.
  network     records the resized `rgbds` and the scaled queries it is given and returns seeded outputs
              (video_util.network_outputs) in the tracker's tuple layout;
  cfg         a settings object with attribute access and `in`; backward_tracking is on, with S_slam == model.S as in every
              shipped config, so the backward branch is not taken.

Inputs come from video_util.make_inputs and are NOT stored: the fixture keeps their digests.  Writes
tests/golden/video_prep.npz; per case c (up 23 x 31 -> 24 x 40 with the static mask, down 60 x 100 -> 24 x 40 with
`use_static`, odd 61 x 97 -> 24 x 40 with the static mask, same 24 x 40 -> 24 x 40):
  c.digest.<input>        float64 [3]
  c.rgbds, c.queries      float32: what the network was handed;   c.f64.rgbds, c.f64.queries   from the float64 run
  c.<return>              tracks, depths, visibilities, dynamic_e (stats['dynamic_e']) as returned;   c.f64.<return>
  gate.c                  max |float32 run - float64 run| of the resized rgbds
and `signature`, of the method.  Only digests of inputs we generated and numeric results are written.

    BATRACK_REFERENCE=<reference checkout> python tests/golden/make_golden_video_prep.py
"""
import inspect
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("BATRACK_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REF:
    sys.exit("set BATRACK_REFERENCE (or pass as the first argument) to the reference checkout")
sys.path[:0] = [os.path.join(HERE, "refstubs"), os.path.join(REF, "main"), REF, ROOT, os.path.join(ROOT, "tests")]
for name, attr in (("main.slam_visualizer", "LEAPVisualizer"), ("main.frontend.md_tracker", "MDTracker")):
    mod = types.ModuleType(name)
    setattr(mod, attr, type(attr, (), {}))
    sys.modules[name] = mod

import main.batrack as ref_batrack                     # noqa: E402  (reference, unmodified)

import video_util as U                                 # noqa: E402

torch.set_num_threads(4)


def run_reference(c, dtype):
    me = U.StandIn(c, dtype, "cpu")
    t = U.case_tensors(c, dtype)
    # the method's `.float()` would take the float64 run back to float32: a float64 tensor that answers it with itself
    rgbds = t["rgbds"]
    if dtype == torch.float64:
        class Keeps64(torch.Tensor):
            def float(self):
                return self.as_subclass(torch.Tensor)
        rgbds = rgbds.as_subclass(Keeps64)
    with torch.no_grad():
        tracks, depths, vis, stats = ref_batrack.BATRACK._compute_sparse_tracks(me, rgbds=rgbds, queries=t["queries"])
    assert len(me.seen) == 1 and me.seen[0]["iters"] == 4 and set(stats) == {"dynamic_e"}
    seen = me.seen[0]
    assert seen["rgbds"].dtype == dtype and tuple(seen["rgbds"].shape) == (1, me.spec["T"], 4, *U.SIZE)
    return dict(rgbds=seen["rgbds"][0], queries=seen["queries"], tracks=tracks, depths=depths, visibilities=vis, dynamic_e=stats["dynamic_e"])


def main():
    f32 = lambda a: a.detach().to(torch.float32).numpy()
    f64 = lambda a: a.detach().to(torch.float64).numpy()
    out = {"signature": np.array(str(inspect.signature(ref_batrack.BATRACK._compute_sparse_tracks)))}
    for c, spec in U.CASES.items():
        r32, r64 = run_reference(c, torch.float32), run_reference(c, torch.float64)
        d = U.make_inputs(**spec)
        for name in U.INPUTS:
            out[f"{c}.digest.{name}"] = U.digest(d[name])
        for name in ("rgbds", "queries") + U.RETURNS:
            assert r32[name].dtype == torch.float32 and r64[name].dtype == torch.float64, (c, name)
            out[f"{c}.{name}"], out[f"{c}.f64.{name}"] = f32(r32[name]), f64(r64[name])
        gate = float((r32["rgbds"].double() - r64["rgbds"]).abs().max())
        assert (gate > 0) if c in U.RESIZING else (gate == 0), (c, gate)
        if c not in U.RESIZING:
            assert torch.equal(r32["rgbds"], U.case_tensors(c)["rgbds"][0])           # the identity size returns the input
        out[f"gate.{c}"] = np.float64(gate)
        depth = r32["rgbds"][:, 3]
        print(f"case {c}: gate {gate:.3e}; resized depth: {int((depth == 0).sum())} zeros, {int(((depth > 0) & (depth <= 0.01)).sum())} in (0, 0.01], "
              f"{int(((depth > 0.01) & (depth < 0.5)).sum())} in (0.01, 0.5)")
    path = os.path.join(HERE, "video_prep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
