"""Trajectory error as the reference reports it: absolute trajectory error (ATE) = RMSE of the
translation part after a Sim(3) (Umeyama) alignment of the estimate onto the reference
trajectory (/root/reference/main/utils.py:337-340: evo `main_ape.ape(..., pose_relation=
translation_part, align=True, correct_scale=True)`, statistic `rmse`).  `evo` is not available
offline; this restates the published closed form (Umeyama 1991) in float64 numpy.

Host-side measurement code (SURVEY.md §8d "ATE"): it consumes trajectories, it is not on the
BA hot path.

Depth accuracy as the reference's global-alignment stage reports it (main/global_refine/model/utils.py:103-116, 203-265):
`compute_errors`, `eval_depth_metric`, `eval_depth` and `print_results` with the reference's signatures, return values and
printed table.  The per-pixel work — the valid set, the exact medians (radix select), the least-squares fit, the clamp and the
eight metrics in float64 — runs on the HIP kernels of include/batrack_depth.h.  Inputs are CUDA tensors or numpy arrays
(uploaded); maps are scored as float32 values, every per-element operation in float64.  CPU tensors raise: there is no CPU
fallback.
"""
import numpy as np


def umeyama(est, ref, with_scale=True):
    """Least-squares similarity (s, R, t) with ref ~ s * R @ est + t; est, ref: [n, 3]."""
    est = np.asarray(est, np.float64)
    ref = np.asarray(ref, np.float64)
    if est.shape != ref.shape or est.ndim != 2 or est.shape[1] != 3 or est.shape[0] < 3:
        raise ValueError("umeyama: two [n>=3, 3] point sets expected")
    mu_e, mu_r = est.mean(0), ref.mean(0)
    xe, xr = est - mu_e, ref - mu_r
    cov = xr.T @ xe / est.shape[0]
    U, d, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    var_e = (xe * xe).sum() / est.shape[0]
    s = float(np.trace(np.diag(d) @ S) / var_e) if with_scale else 1.0
    t = mu_r - s * R @ mu_e
    return s, R, t


def camera_centres(poses):
    """World-to-camera poses [n, 7] = (t, q xyzw) -> camera centres in the world, -R^T t
    (the reference saves `poses.inv()`, batrack.py:1086-1087)."""
    p = np.asarray(poses, np.float64)
    t, q = p[:, :3], p[:, 3:] / np.linalg.norm(p[:, 3:], axis=1, keepdims=True)
    qv, w = -q[:, :3], q[:, 3:4]                      # conjugate: rotate by R^T
    uv = 2.0 * np.cross(qv, t)
    return -(t + w * uv + np.cross(qv, uv))


def ate_rmse(est_xyz, ref_xyz, align=True, correct_scale=True):
    """APE-RMSE of the translation part (utils.py:337-340)."""
    est = np.asarray(est_xyz, np.float64)
    ref = np.asarray(ref_xyz, np.float64)
    if align:
        s, R, t = umeyama(est, ref, with_scale=correct_scale)
        est = s * est @ R.T + t
    return float(np.sqrt(((est - ref) ** 2).sum(1).mean()))


# ---------------------------------------------------------------------- depth metrics (model/utils.py:103-116, 203-265)
_SCALING = {"median": 1, "lstsq": 2}                  # any other string: no scaling, as the reference's elif chain
METRICS = ("abs_rel", "sq_rel", "log10", "rmse", "rmse_log", "a1", "a2", "a3")


def _device_of(*xs):
    import torch
    for x in xs:
        if isinstance(x, torch.Tensor):
            if x.device.type != "cuda":
                raise RuntimeError("batrack_amd.evaluation: tensors must be on the GPU (no CPU fallback in batrack_amd)")
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _flat(x, np_dtype, dev):
    """A CUDA tensor (kept on its device) or an array (uploaded) as a flat contiguous tensor of `np_dtype`."""
    import torch
    if isinstance(x, torch.Tensor):
        dt = torch.from_numpy(np.zeros(0, np_dtype)).dtype
        return x.detach().to(device=dev, dtype=dt).reshape(-1).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np_dtype), device=dev)


def depth_metrics(gt, pred, mask=None, depth_min=1e-2, depth_max=1e2, scaling="median"):
    """bt_depth_metrics on one pair of arrays: numpy float64 [11] = the eight metrics (METRICS order), the valid count,
    the ratio (median) or s (lstsq) or 1, and t (lstsq) or 0.  valid = mask & (gt > depth_min) & (gt < depth_max)."""
    import torch
    from . import _lib
    if scaling in ("la2d", "lad"):
        raise NotImplementedError(f"scaling {scaling!r}: the reference's iterative scipy / Adam fits (utils.py:119-185) are not "
                                  "ported; use 'median', 'lstsq' or no scaling")
    dev = _device_of(gt, pred, mask)
    g, p = _flat(gt, np.float32, dev), _flat(pred, np.float32, dev)
    if g.numel() != p.numel():
        raise ValueError(f"gt and pred hold {g.numel()} and {p.numel()} elements")
    m = None
    if mask is not None:
        m = _flat(mask.bool() if isinstance(mask, torch.Tensor) else np.asarray(mask, bool), np.uint8, dev)
        if m.numel() != g.numel():
            raise ValueError("mask and gt differ in size")
    L = _lib.lib()
    n = g.numel()
    wb = L.bt_depth_metrics_workspace_bytes(n)
    if wb < 0:
        _lib.check(int(wb), "bt_depth_metrics_workspace_bytes")
    ws = torch.empty(int(wb), dtype=torch.uint8, device=dev)
    out = torch.empty(11, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.bt_depth_metrics(g.data_ptr(), p.data_ptr(), None if m is None else m.data_ptr(), n, float(depth_min),
                                      float(depth_max), _SCALING.get(scaling, 0) if isinstance(scaling, str) else 0,
                                      ws.data_ptr(), out.data_ptr(), st), "bt_depth_metrics")
        return out.cpu().numpy()                      # the one synchronisation


def compute_errors(gt, pred, min_depth, max_depth, scaling="median"):
    """utils.py:203-240 on the HIP kernels: (abs_rel, sq_rel, log10, rmse, rmse_log, a1, a2, a3) of pred against gt after
    median / lstsq / no scaling and clamping to [min_depth, max_depth].  The reference calls it with the valid elements only
    (eval_depth_metric); so must a caller here: an element whose gt is not inside (min_depth, max_depth) raises ValueError
    (the kernel would leave it out).  `pred` is not modified."""
    r = depth_metrics(gt, pred, None, min_depth, max_depth, scaling)
    n = int(np.asarray(gt).size) if not hasattr(gt, "numel") else int(gt.numel())
    if int(r[8]) != n:
        raise ValueError(f"compute_errors: {n - int(r[8])} of {n} gt values are not inside (min_depth, max_depth); "
                         "pass the valid elements only, or use eval_depth_metric")
    return tuple(np.float64(v) for v in r[:8])


def print_results(exp_name, results):
    """utils.py:243-250."""
    print(f"\n {exp_name}")
    print("\n  {:>10}|".format("depth") + ("{:>8} | " * 8).format(*METRICS))
    for key, value in results.items():
        print(("{:>10} " + "&{: 8.3f}  " * 8).format(key, *value.tolist()) + "\\\\")


def eval_depth_metric(gt_depth, pred_depth_dict, mask, exp_name="", depth_min=1e-2, depth_max=1e2, scaling="median"):
    """utils.py:253-265: for every entry of `pred_depth_dict` the eight metrics over mask & (gt > depth_min) & (gt < depth_max),
    as a numpy float64 array; prints the table and returns the dict.  `mask` None: every element."""
    results = {}
    for key, value in pred_depth_dict.items():
        results[key] = np.array(depth_metrics(gt_depth, value, mask, depth_min, depth_max, scaling)[:8])
    print_results(exp_name, results)
    return results


def eval_depth(ba_model, depth_min=1e-2, depth_max=1e2, scaling="median", scene_name="all"):
    """utils.py:103-116: the refined maps `ba_model.scaled_dmaps` against `ba_model.results['dmaps_gt']` (channel 0), masked
    to 1e-2 < gt < 1e2 and then to (depth_min, depth_max).  gt is scored as float32 values."""
    import torch
    gt_np = np.asarray(ba_model.results["dmaps_gt"])[..., 0]
    pred = ba_model.scaled_dmaps[:, 0].detach()
    gt = torch.as_tensor(np.ascontiguousarray(gt_np, dtype=np.float32), device=pred.device)
    mask = (gt > 1e-2) & (gt < 1e2)
    return eval_depth_metric(gt, {"final": pred}, mask, exp_name=scene_name, depth_min=depth_min, depth_max=depth_max, scaling=scaling)
