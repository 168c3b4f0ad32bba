#!/usr/bin/env python3
"""Golden vectors for the tracker's window loop: the reference's UNMODIFIED `MDTracker.forward`
(main/frontend/md_tracker.py:416-671) on torch-CPU, where the reference checkout is at hand.  The method is called unbound
on a plain object (tests/tracker_window_util.StandIn) that carries the attributes it reads, once in float32 and once in
float64 (default dtype float64, so that the tensors the method creates itself are float64 too).

Stand-ins.  tests/golden/refstubs first on sys.path supplies the modules the reference imports and this path never calls.
  fnet                returns seeded maps (tracker_window_util.fnet_maps), whatever its input is;
  forward_iteration   records what it is given and returns prepared, seeded outputs (tracker_window_util.iteration_outputs);
  embedConv           a real Conv2d with seeded weights and a non-zero bias;   embed3d   the reference's Embedder_Fourier.

Inputs come from tracker_window_util.make_inputs and are NOT stored: the fixture keeps their digests.  Writes
tests/golden/tracker_window.npz; per case c and window k (a call of forward_iteration), from the float32 run:
  c.digest.<input>     float64 [3]
  c.k.dmaps, .feat_init, .coords_init, .coords_dyn_init, .vis_init, .track_mask      as handed to forward_iteration
  c.k.fmaps            the frames of fmaps the window computed (all S of the first window, the new half of a slide)
  c.<return>           traj_e, feat_init, depth_e, traj_static_e, vis_e, dynamic_e as returned;   c.rgbds_digest  of rgbds afterwards
  c.d_range            (d_near, d_far) as the method left them on the object
from the float64 run, for the restatement to be checked against: c.k.f64.<the same names> (fmaps: every 32nd element) and
c.f64.<return>;  gate.c.<name>: max over the windows of |float32 run - float64 run|;  `signature`: of MDTracker.forward.
Only digests of inputs we generated and numeric results are written.

    BATRACK_REFERENCE=<reference checkout> python tests/golden/make_golden_tracker_window.py
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

import main.frontend.md_tracker as md                                        # noqa: E402  (reference, unmodified)
from main.frontend.core.embeddings import Embedder_Fourier                   # noqa: E402

import tracker_window_util as U                                              # noqa: E402

torch.set_num_threads(4)


def run_reference(c, dtype):
    embed3d = Embedder_Fourier(input_dim=3, max_freq_log2=10.0, N_freqs=10, include_input=True)    # as the model builds it: in float32
    assert embed3d.freq_bands == U.FREQS
    torch.set_default_dtype(dtype)
    try:
        me = U.StandIn(c, dtype, "cpu", embed3d)
        T = U.case_tensors(c, dtype)
        with torch.no_grad():
            ret = md.MDTracker.forward(me, T["rgbds"], T["queries"], iters=4)
    finally:
        torch.set_default_dtype(torch.float32)
    assert ret[6] is None and len(ret) == 7
    S, windows, call = me.S, [], 0
    # which encoder call belongs to which window: every window calls the encoder once, a window without queries included
    ind, k = 0, 0
    for call in range(me.fnet_calls):
        n = sum(f < ind + S for f in me.spec["first"])
        if n:
            seen = dict(me.seen[k])
            assert seen["fmaps"].shape[1] == S
            seen["fmaps"] = seen["fmaps"][0, U.computed_frames(call, S)]
            windows.append(seen)
            k += 1
        ind += S // 2
    assert k == len(me.seen)
    return dict(windows=windows, ret=dict(zip(U.RETURNS, ret[:6])), rgbds=T["rgbds"], d_range=(me.d_near, me.d_far))


def main():
    f32 = lambda a: a.detach().to(torch.float32).numpy()
    f64 = lambda a: a.detach().to(torch.float64).numpy()
    out = {"signature": np.array(str(inspect.signature(md.MDTracker.forward)))}
    for c, spec in U.CASES.items():
        r32, r64 = run_reference(c, torch.float32), run_reference(c, torch.float64)
        d = U.make_inputs(**spec)
        for name in U.INPUTS:
            out[f"{c}.digest.{name}"] = U.digest(d[name])
        out[f"{c}.rgbds_digest"] = U.digest(f32(r32["rgbds"]))
        out[f"{c}.d_range"] = np.array(r32["d_range"], np.float64)
        assert r32["d_range"] == r64["d_range"]
        gates = {}
        for k, (a, b) in enumerate(zip(r32["windows"], r64["windows"])):
            for name in U.WINDOW_KEYS + ("fmaps",):
                if name == "track_mask":
                    assert torch.equal(a[name], b[name])
                    out[f"{c}.{k}.{name}"] = a[name].numpy()
                    continue
                assert a[name].dtype == torch.float32
                out[f"{c}.{k}.{name}"] = f32(a[name])
                out[f"{c}.{k}.f64.{name}"] = f64(b[name]).ravel()[::U.F64_STEP] if name == "fmaps" else f64(b[name])
                gates[name] = max(gates.get(name, 0.0), float((a[name].double() - b[name].double()).abs().max()))
        for name in U.RETURNS:
            a, b = r32["ret"][name], r64["ret"][name]
            out[f"{c}.{name}"], out[f"{c}.f64.{name}"] = f32(a), f64(b)
            gates[name] = float((a.double() - b.double()).abs().max())
        for name, g in gates.items():
            out[f"gate.{c}.{name}"] = np.float64(g)
        print(f"case {c}: {len(r32['windows'])} windows, max |fmaps| {max(float(w['fmaps'].abs().max()) for w in r32['windows']):.2f}; gates "
              + ", ".join(f"{n} {g:.2e}" for n, g in gates.items()))
    path = os.path.join(HERE, "tracker_window.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
