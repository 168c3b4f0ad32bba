"""A numpy restatement of the reference's depth metrics (main/global_refine/model/utils.py:187-265) as the kernels define
them (include/batrack_depth.h): float32 values, every per-element operation in float64, the limits compared and clamped as
float32 numbers.  Returns the 11 numbers of bt_depth_metrics."""
import numpy as np


def np_depth_metrics(gt, pred, mask=None, depth_min=1e-2, depth_max=1e2, scaling="median"):
    g = np.asarray(gt, np.float32).astype(np.float64).ravel()
    p = np.asarray(pred, np.float32).astype(np.float64).ravel()
    lo, hi = float(np.float32(depth_min)), float(np.float32(depth_max))
    valid = (g > lo) & (g < hi) & (np.ones(g.shape, bool) if mask is None else np.asarray(mask, bool).ravel())
    g, p = g[valid], p[valid]
    s, t = 1.0, 0.0
    with np.errstate(all="ignore"):
        if scaling == "median":
            s = np.median(g) / np.median(p) if g.size else np.nan
            p = p * s
        elif scaling == "lstsq" and g.size:
            s, t = np.linalg.lstsq(np.stack([p, np.ones_like(p)], 1), g, rcond=None)[0]
            p = s * p + t
        p[p < lo] = lo
        p[p > hi] = hi
        th = np.maximum(g / p, p / g)
        e = g - p
        m = [np.mean(np.abs(e) / g), np.mean(e ** 2 / g), np.mean(np.abs(np.log10(p) - np.log10(g))), np.sqrt(np.mean(e ** 2)),
             np.sqrt(np.mean((np.log(g) - np.log(p)) ** 2)), (th < 1.25).mean(), (th < 1.25 ** 2).mean(), (th < 1.25 ** 3).mean()]
    return np.array([float(x) for x in m] + [float(g.size), float(s), float(t)])
