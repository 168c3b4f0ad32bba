#!/usr/bin/env python3
"""Golden vectors for the tracker's refinement iteration: the reference's UNMODIFIED `MDTracker.forward_iteration`
(main/frontend/md_tracker.py:181-413) and `sample_pos_embed` (:49-61) on torch-CPU, where the reference checkout is at
hand.  The method is called unbound on a plain object that carries the attributes it reads.

Stand-ins.  tests/golden/refstubs first on sys.path supplies empty `timm` and `torchvision` modules, which the reference's
blocks.py imports and this path never calls; `einops` is installed.  On the object:
  updateformer, updateformer_dyn   record their input x and return a PREPARED, seeded delta that does not depend on x.
                                   (With a delta computed from x the reference's own float32 and float64 runs drift apart
                                   within a few iterations: the 968 rad/px flow embedding is chaotic.  With prepared deltas
                                   the chain is well conditioned.)
  ffeat_updater                    the real Linear + GELU, wrapped to record what it returns: the feature state after a
                                   call is that plus the state before, the one float add the reference does.
  vis_predictor, motion_label_block   record the final features and coordinates (checked against the states rebuilt from
                                   the recorded pieces, bit for bit); the latter returns a prepared motion logit.
In the tracker module's namespace `sample_pos_embed` and `CorrBlock` are wrapped to record what they return; the
reference's own code runs inside both.

Inputs come from tests/track_iter_util.make_inputs (seeded, rounded to float32) and are NOT stored: the fixture keeps
their digests.  Writes tests/golden/track_iter.npz; per case c of track_iter_util.CASES and recorded call k (the iters
calls of updateformer, then the static calls of updateformer_dyn), from the reference's float32 run:
  c.digest.<input>      float64 [3]
  c.pos, c.pos_static   [N, 456]   what sample_pos_embed returned, transposed (pos_static: cases with static calls)   c.time  [S, 456]
  c.k.flow     [N, S, 130]   the flow columns of x             c.k.copy_digest   of x[..., 130:], which the generator asserts
  c.k.ffeats   [S, N, 128]   the features after the update                       equal (cat(...) + pos) + time bit for bit
  c.k.state    [S, N, 3]     coords (static calls: coords_dyn) after the update  c.k.tail_digest   of x[..., 326:] (features, mask)
  c.k.out      [S, N, 3]     the output coordinates of the call
  c.vis_e, c.dynamic_e       as returned
  gate.c.k.flow / .ffeats / .out   max |float32 run - float64 run| of the reference on the same inputs
and `signatures`: str(inspect.signature(...)) of sample_pos_embed and MDTracker.forward_iteration.
Only digests of inputs we generated and numeric results are written.

    BATRACK_REFERENCE=<reference checkout> python tests/golden/make_golden_track_iter.py
"""
import functools
import inspect
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("BATRACK_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REF:
    sys.exit("set BATRACK_REFERENCE (or pass as the first argument) to the reference checkout")
sys.path[:0] = [os.path.join(HERE, "refstubs"), REF, os.path.join(ROOT, "tests")]

import main.frontend.md_tracker as md                                        # noqa: E402  (reference, unmodified)
from main.frontend.core.embeddings import get_1d_sincos_pos_embed_from_grid   # noqa: E402

import track_iter_util as U                                                  # noqa: E402

torch.set_num_threads(4)
REF_SAMPLE_POS_EMBED, REF_CORRBLOCK = md.sample_pos_embed, md.CorrBlock


class Prepared(nn.Module):
    """Records its inputs; returns the next prepared output."""
    def __init__(self, outputs):
        super().__init__()
        self.outputs, self.seen = list(outputs), []

    def forward(self, *args):
        self.seen.append([a.detach().clone() for a in args])
        return self.outputs[len(self.seen) - 1]


class Recording(nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.returned = inner, []

    def forward(self, x):
        y = self.inner(x)
        self.returned.append(y.detach().clone())
        return y


def run_reference(c, dtype):
    spec = U.CASES[c]
    d = U.make_inputs(**spec)
    t = lambda a: torch.as_tensor(a, dtype=dtype)
    S, N, it, st = spec["S"], spec["N"], spec["iters"], spec["static"]

    def lin(w, b):
        m = nn.Linear(w.shape[1], w.shape[0]).to(dtype)
        m.weight.data.copy_(t(w))
        m.bias.data.copy_(t(b))
        return m
    norm = nn.GroupNorm(1, U.C).to(dtype)
    norm.weight.data.copy_(t(d["gamma"]))
    norm.bias.data.copy_(t(d["beta"]))
    deltas = t(d["deltas"])
    pos_rec, corr_rec = [], []

    def sample_pos_embed(grid_size, embed_dim, coords):
        out = REF_SAMPLE_POS_EMBED(grid_size, embed_dim, coords)
        pos_rec.append(out.detach().clone())
        return out

    class CorrBlock(REF_CORRBLOCK):
        def sample(self, coords):
            out = super().sample(coords)
            corr_rec.append(out.detach().clone())
            return out

    me = types.SimpleNamespace(
        corr_levels=U.LEVELS, corr_radius=U.RADIUS, input_dim=U.E, latent_dim=U.C, fix_track_mask=bool(spec["fix"]),
        zeroMLPflow=lin(d["w_flow"], d["b_flow"]), norm=norm,
        ffeat_updater=Recording(nn.Sequential(lin(d["w_u"], d["b_u"]), nn.GELU())),
        updateformer=Prepared(deltas[:it]), updateformer_dyn=Prepared(deltas[it:]),
        vis_predictor=Prepared([torch.zeros(S * N, 1, dtype=dtype)]), motion_label_block=Prepared([t(d["dyn_logit"])]),
        stride=int(d["scale"]["stride"]), Dz=int(d["scale"]["Dz"]), d_near=d["scale"]["d_near"], d_far=d["scale"]["d_far"],
        use_log_depth=d["scale"]["use_log_depth"], dynamic_mask_detach=True, static_iters=st)
    me.depth_process_inv = functools.partial(md.MDTracker.depth_process_inv, me)
    md.sample_pos_embed, md.CorrBlock = sample_pos_embed, CorrBlock
    try:
        with torch.no_grad():
            ret = md.MDTracker.forward_iteration(me, t(d["fmaps"]), None, t(d["coords_init"]), t(d["coords_dyn_init"]),
                                                 feat_init=t(d["feat_init"]), vis_init=t(d["vis_init"]), track_mask=t(d["track_mask"]),
                                                 iters=it)
    finally:
        md.sample_pos_embed, md.CorrBlock = REF_SAMPLE_POS_EMBED, REF_CORRBLOCK
    coord_pred, depth_pred, static_pred, vis_e, dynamic_e, feat_back = ret
    assert feat_back.shape == (1, S, N, U.C) and len(coord_pred) == it and len(static_pred) == st and len(pos_rec) == 2

    # ---- the pieces, per call
    T = U.case_tensors(c, dtype)
    time = torch.from_numpy(get_1d_sincos_pos_embed_from_grid(U.E, torch.linspace(0, S - 1, S).reshape(S, 1).numpy())).float()
    pos = [p[0].t().contiguous() for p in pos_rec]
    xs = [s[0][0] for s in me.updateformer.seen + me.updateformer_dyn.seen]
    coords, coords_dyn, ffeats, ffeats_static = T["coords"].clone(), T["coords_dyn"].clone(), T["ffeats"].clone(), T["ffeats"].clone()
    calls = []
    for k in range(it + st):
        x, static = xs[k], k >= it
        assert x.shape == (N, S, U.E)
        fe = ffeats_static if static else ffeats
        copy = torch.cat([corr_rec[k][0].permute(1, 0, 2), fe.permute(1, 0, 2), U.mask_columns(T["track_mask"], T["vis"], spec["fix"])], -1)
        want = (copy + pos[static][:, None, U.F:]) + time[None, :, U.F:]
        assert torch.equal(x[..., U.F:], want), (c, k)                       # the copy columns, bit for bit
        upd = me.ffeat_updater.returned[k].reshape(N, S, U.C).permute(1, 0, 2)
        dxyz = deltas[k, 0, :, :, :3].permute(1, 0, 2)
        if static:
            ffeats_static, coords_dyn = upd + ffeats_static, coords_dyn + dxyz
            out = static_pred[k - it][0]
        else:
            ffeats, coords = upd + ffeats, coords + dxyz
            out = torch.cat([coord_pred[k][0], depth_pred[k][0]], -1)
        calls.append(dict(x=x, flow=x[..., :U.F], ffeats=(ffeats_static if static else ffeats).clone(),
                          state=(coords_dyn if static else coords).clone(), out=out))
    seen_ffeats, seen_coords = me.motion_label_block.seen[0]
    assert torch.equal(seen_ffeats[0], ffeats) and torch.equal(seen_coords[0], coords)       # the rebuilt states are the reference's
    assert torch.equal(me.vis_predictor.seen[0][0].reshape(S, N, U.C), ffeats)
    return dict(calls=calls, pos=pos[0], pos_static=pos[1], time=time, vis_e=vis_e, dynamic_e=dynamic_e, inputs=d)


def main():
    f32 = lambda a: a.detach().to(torch.float32).numpy()
    out = {"signatures": np.array([str(inspect.signature(f)) for f in (md.sample_pos_embed, md.MDTracker.forward_iteration)])}
    for c, spec in U.CASES.items():
        r32, r64 = run_reference(c, torch.float32), run_reference(c, torch.float64)
        for name in U.INPUTS:
            out[f"{c}.digest.{name}"] = U.digest(r32["inputs"][name])
        assert r32["pos"].dtype == torch.float32 and torch.equal(r32["pos"], r64["pos"])
        for name in ("pos", "pos_static", "time", "vis_e", "dynamic_e"):
            if name != "pos_static" or spec["static"]:                      # no static call, no x that holds it
                out[f"{c}.{name}"] = f32(r32[name])
        line = []
        for k, (a, b) in enumerate(zip(r32["calls"], r64["calls"])):
            for name in ("flow", "ffeats", "state", "out"):
                out[f"{c}.{k}.{name}"] = f32(a[name])
            out[f"{c}.{k}.copy_digest"] = U.digest(f32(a["x"][..., U.F:]))
            out[f"{c}.{k}.tail_digest"] = U.digest(f32(a["x"][..., U.F + U.LRR:]))
            for name in ("flow", "ffeats", "out"):
                out[f"gate.{c}.{k}.{name}"] = np.float64((a[name].double() - b[name]).abs().max())
            line.append("call %d: gates flow %.2e ffeats %.2e out %.2e, state f32 vs f64 %.1e" % (
                k, out[f"gate.{c}.{k}.flow"], out[f"gate.{c}.{k}.ffeats"], out[f"gate.{c}.{k}.out"],
                (a["state"].double() - b["state"]).abs().max()))
        print(f"case {c} (S={spec['S']}, N={spec['N']}): " + "; ".join(line))
    path = os.path.join(HERE, "track_iter.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
