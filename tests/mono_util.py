"""The mono-depth alignment (main/mono_depth/get_mono_depth.py:52-140) restated in numpy from its formulas, with the
intermediates bt_mono_align reports (include/batrack_depth.h): per-frame scales s and shifts c, the aligns (a_s, a_c, n) and
k.  Everything runs in the metric depth's dtype D as numpy's promotion rules (NEP 50) put it: the Python scalars of the
formulas take D, a float32 disparity widens where it meets a float64 value."""
import numpy as np


def restate(mono, metric):
    d = np.asarray(mono).astype(np.float32)
    m = np.asarray(metric)
    D = m.dtype.type
    T = m.shape[0]
    s, c = np.empty(T, D), np.empty(T, D)
    with np.errstate(all="ignore"):
        for t in range(T):
            g = D(1) / (m[t] + D(1e-8))
            g[(m[t] < D(2)) & (d[t] < np.float32(0.02))] = D(0.01)
            num = g - np.median(g) + D(1e-8)                                # D
            den = d[t] - np.median(d[t]) + np.float32(1e-8)                 # float32
            s[t] = np.median(num / den)
            c[t] = np.median(g - s[t] * d[t])
        p = s * c
        k = int(np.argmin(np.abs(p - np.median(p))))
        y = s[k] * d + c[k]                                                 # D (a numpy scalar is strong)
        n = np.percentile(y, 98) / D(2)
        depth = np.clip(D(1) / ((D(1) / n) * y), D(1e-4), D(1e4))
        depth[depth < D(1e-2)] = D(0)
    return depth, s, c, np.array([s[k], c[k], n], D), k


def percentile_gamma(n_elems, dtype):
    """numpy's gamma for the 98th percentile of n_elems values of `dtype` (method 'linear'): the fractional part of (n - 1) q."""
    q = np.true_divide(98, dtype(100))
    v = (n_elems - 1) * np.asanyarray(q)
    return float(v - np.floor(v))
