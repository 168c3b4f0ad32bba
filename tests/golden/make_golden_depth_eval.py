#!/usr/bin/env python3
"""Golden vectors for the output of the reference's dense global-alignment stage and its depth metrics: runs the reference's
UNMODIFIED main/global_refine/model/{refine_net,trainer,utils}.py on inputs we generate, in this container only.
`pypose` is absent: tests/golden/refstubs/pypose stands in (as for make_golden_ga.py).  Writes tests/golden/depth_eval.npz:
  sd.*     RefineNet.scaled_dmaps (refine_net.py:408-416) on T = 6 maps of 48 x 64, scale grids 4 x 4 and 3 x 5, non-zero
           frame_shifts_; float64 arithmetic on float32-representable inputs
  ce.*     eval_depth_metric / compute_errors (utils.py:203-265) with median, lstsq and no scaling, on inputs rounded to float32
           first (so that only the order of the float64 arithmetic differs), odd and even valid counts, heavy ties, a mask and
           preds outside [depth_min, depth_max]; with the valid count, np.median's ratio and np.linalg.lstsq's (s, t)
  loop.*   20 iterations of global_alignment_loop (trainer.py:23-77) on the total run_global_refine.py optimises, for
           (fixed_pose, fixed_K) = (False, False) and (True, True): the lr of every iteration, the losses and the final
           parameters (float64 reference)
Only inputs we generated and numeric outputs are written.

    python tests/golden/make_golden_depth_eval.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ga as base              # noqa: E402  (inputs, the __init__-free construction; puts the stubs and the reference on sys.path)
import make_golden_ga_total as total       # noqa: E402
import pypose as pp                        # noqa: E402  (stand-in)
from model import trainer                  # noqa: E402  (reference, unmodified)
from model.refine_net import RefineNet     # noqa: E402
from model.utils import eval_depth_metric  # noqa: E402

SCALING = {"none": 0, "median": 1, "lstsq": 2}


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def scaled_dmaps(out, rng):
    T, H, W = 6, 48, 64
    dm = f32(rng.uniform(0.5, 12.0, (T, 1, H, W)))
    out["sd.dmaps"] = dm.astype(np.float32)
    for tag, (gh, gw) in (("g44", (4, 4)), ("g35", (3, 5))):
        net = object.__new__(RefineNet)
        torch.nn.Module.__init__(net)
        net.H, net.W, net.scale_mode = H, W, "exp"
        fs = f32(rng.standard_normal((T, gh, gw)) * 2.0)
        sh = f32(rng.uniform(-0.03, 0.05, T))
        net.frame_scales_ = torch.nn.Parameter(torch.as_tensor(fs))
        net.frame_shifts_ = torch.as_tensor(sh)
        net.dmaps = torch.as_tensor(dm)
        with torch.no_grad():
            out[f"sd.{tag}.frame_scales_"] = fs.astype(np.float32)
            out[f"sd.{tag}.frame_shifts_"] = sh.astype(np.float32)
            out[f"sd.{tag}.scaled"] = net.scaled_dmaps.numpy().astype(np.float32)     # (float64 result; stored to 6e-8)


def metric_cases(rng, out):
    """The inputs (ce.in.*, each stored once) and the cases: (name, gt key, pred key, mask key, depth_min, depth_max, scaling)."""
    shape = (3, 29, 41)
    gt = f32(np.exp(rng.uniform(np.log(0.1), np.log(80.0), shape)))
    pred = f32(gt * 1.7 * np.exp(0.25 * rng.standard_normal(shape)))
    pred.flat[::97] = 0.05                                                    # below depth_min after scaling
    pred.flat[5::131] = 400.0                                                 # above depth_max
    mask = rng.uniform(size=shape) < 0.8
    arrays = dict(gt=gt, pred=pred, mask=mask, ties_gt=f32(np.round(gt * 2.0) / 2.0 + 0.5),      # ~160 distinct values
                  ties_pred=f32(np.round(pred * 4.0) / 4.0 + 0.25), const=np.full(shape, 3.0), ones=np.ones(shape, bool),
                  pred_floor=f32(np.maximum(pred, 0.2)))
    valid = mask & (gt > 0.25) & (gt < 64.0)
    arrays["mask_flip"] = mask.copy()
    arrays["mask_flip"].flat[np.flatnonzero(valid)[0]] = False                # one valid element fewer: the other parity
    par = {int(valid.sum()) % 2: "mask", 1 - int(valid.sum()) % 2: "mask_flip"}
    cases = []
    for scaling in ("median", "lstsq", "none"):
        cases.append((f"{scaling}_odd", "gt", "pred", par[1], 0.25, 64.0, scaling))
        cases.append((f"{scaling}_even", "gt", "pred", par[0], 0.25, 64.0, scaling))
    cases.append(("median_ties", "ties_gt", "ties_pred", "mask", 0.25, 64.0, "median"))
    cases.append(("median_ties_nomask", "ties_gt", "ties_pred", "ones", 0.5, 32.0, "median"))
    cases.append(("lstsq_ties", "ties_gt", "ties_pred", "mask", 0.25, 64.0, "lstsq"))
    cases.append(("median_const_pred", "gt", "const", "mask", 0.25, 64.0, "median"))
    cases.append(("lstsq_const_pred", "gt", "const", "mask", 0.25, 64.0, "lstsq"))     # singular: the minimum-norm solution
    cases.append(("median_default_limits", "gt", "pred_floor", "mask", 1e-2, 1e2, "median"))
    for k, v in arrays.items():
        out[f"ce.in.{k}"] = v if v.dtype == bool else v.astype(np.float32)
    return arrays, cases


def depth_metrics(out):
    arrays, cases = metric_cases(np.random.default_rng(11), out)
    for name, kg, kp, km, dmin, dmax, scaling in cases:
        gt, pred, mask = arrays[kg], arrays[kp], arrays[km]
        with contextlib.redirect_stdout(io.StringIO()):
            res = eval_depth_metric(gt, {"final": pred}, mask, exp_name=name, depth_min=dmin, depth_max=dmax, scaling=scaling)
        valid = mask & (gt > dmin) & (gt < dmax)
        gv, pv = gt[valid], pred[valid]
        aux = [float(valid.sum()), 1.0, 0.0]
        if scaling == "median":
            aux[1] = float(np.median(gv) / np.median(pv))
        elif scaling == "lstsq":
            A = np.hstack([pv.reshape(-1, 1), np.ones((pv.size, 1))])
            st = np.linalg.lstsq(A, gv.reshape(-1, 1), rcond=None)[0]
            aux[1:] = [float(st[0, 0]), float(st[1, 0])]
        out[f"ce.{name}.inputs"] = np.array([kg, kp, km])
        out[f"ce.{name}.limits"] = np.array([dmin, dmax])
        out[f"ce.{name}.scaling"] = np.int64(SCALING[scaling])
        out[f"ce.{name}.metrics"] = np.asarray(res["final"], np.float64)
        out[f"ce.{name}.aux"] = np.array(aux)
    out["ce.names"] = np.array([c[0] for c in cases])


def loop(out):
    d = base.make_inputs(T=10, N=32, S=5, seed=4)
    d["frame_scales_"] = np.ones_like(d["frame_scales_"])                     # the reference's initial values (refine_net.py:42-43)
    d["trajs_scales"] = np.ones_like(d["trajs_scales"])
    for k, v in d.items():
        out[f"loop.in.{k}"] = np.array(v)
    for tag, fixed in (("free", False), ("fixed", True)):
        # (a fresh copy per run: the reference's parameters share memory with the arrays they are built from, Adam steps them in place)
        net, _ = total.build({k: np.array(v) for k, v in d.items()}, torch.float64, total.WEIGHTS, True)
        net.pose = pp.Parameter(torch.as_tensor(d["pose"], dtype=torch.float64))
        lrs, losses = [], []
        inner = trainer.global_alignment_iter

        def rec(*a, **k):
            loss, lr = inner(*a, **k)
            losses.append(loss)
            lrs.append(lr)
            return loss, lr
        trainer.global_alignment_iter = rec
        try:
            last = trainer.global_alignment_loop(net, lr=1e-2, niter=20, schedule="cosine", lr_min=1e-6, fixed_pose=fixed, fixed_K=fixed)
        finally:
            trainer.global_alignment_iter = inner
        out[f"loop.{tag}.lr"] = np.array(lrs)
        out[f"loop.{tag}.loss"] = np.array(losses)
        out[f"loop.{tag}.last"] = np.float64(last)
        out[f"loop.{tag}.trajs_scales"] = net.trajs_scales.detach().numpy()
        out[f"loop.{tag}.frame_scales_"] = net.frame_scales_.detach().numpy()
        out[f"loop.{tag}.pose"] = net.pose.tensor().detach().numpy()
        out[f"loop.{tag}.K"] = net.K.detach().numpy()


def main():
    torch.manual_seed(0)
    out = {}
    scaled_dmaps(out, np.random.default_rng(5))
    depth_metrics(out)
    loop(out)
    path = os.path.join(HERE, "depth_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        if k.endswith(".metrics") or k.endswith(".aux"):
            print(k, out[k])
    for tag in ("free", "fixed"):
        print(tag, out[f"loop.{tag}.loss"][[0, -1]])


if __name__ == "__main__":
    main()
