#!/usr/bin/env python3
"""Golden vectors for the mono-depth alignment (main/mono_depth/get_mono_depth.py:21-150): runs the reference's UNMODIFIED
align_depth on scenes we generate, where the reference checkout is at hand, with refstubs/cv2.py standing in for OpenCV
(imread gives an image of the recorded size; resize is the identity between equal sizes).  Writes tests/golden/mono_depth.npz,
for every case `<case>`:
  .mono       the disparities written as <name>.npy files [Tm, H, W] float32
  .metric     the metric depths written as <name>.npz 'depth' [Tn, H, W] (float32 or float64), .intrinsics their 'intrinsics'
  .image_hw   the size of the scene's image;  .names  the file names (without extension), the same for both lists
  .depth      the <name>.npy files the reference wrote [min(Tm, Tn), H, W];  .K  the <name>_intrinsics.npy (all equal)
and `signatures`, the reference's signatures of intrinsics_to_fov, align_depth and align_davis_demo (JSON).
Cases: even (24 x 32, T = 4: pixels at and around float32(0.02) and m = 2, a sky-dominated frame, m of 0, +-inf, negative and
-1e-8), odd (23 x 31, T = 3), f64 (float64 metric), odd_f64, single (T = 1), ties (few distinct values; frames 1 and 2 equal,
so argmin meets a tie), nan_metric (NaN in metric frame 1: finite output), nan_mono (NaN in mono frame 1: all NaN), mismatch
(5 mono files, 4 metric files).  The percentile's gamma is >= 0.5 for some and < 0.5 for others.

    python tests/golden/make_golden_mono_depth.py
"""
import contextlib
import inspect
import io
import json
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/main/mono_depth"
sys.path[:0] = [os.path.join(HERE, "refstubs"), REF]
import cv2  # noqa: E402  (refstubs/cv2.py)
import get_mono_depth as ref  # noqa: E402  (reference, unmodified)


def frames(rng, T, H, W, dt):
    """A DepthAnything-like disparity d in (0, 1) and a UniDepth-like metric depth m ~ 1 / (a d + b), with noise."""
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    d = np.empty((T, H, W), np.float32)
    m = np.empty((T, H, W), dt)
    for t in range(T):
        base = 0.05 + 0.9 * (0.5 + 0.5 * np.sin(2.5 * x + 1.5 * y + t))
        dd = np.clip(base * (1 + 0.1 * rng.standard_normal((H, W))), 1e-3, 1.0)
        a, b = rng.uniform(0.5, 2.0), rng.uniform(0.01, 0.1)
        d[t] = dd
        m[t] = 1.0 / (a * dd + b) * (1 + 0.05 * rng.standard_normal((H, W)))
    return d, m


def boundaries(rng, d, m, t):
    """Pixels of frame t at and around d = float32(0.02) and m = 2, in every combination."""
    f2 = np.float32(0.02)
    ds = [np.nextafter(f2, np.float32(0)), f2, np.nextafter(f2, np.float32(1))]
    two = m.dtype.type(2.0)
    ms = [np.nextafter(two, m.dtype.type(0)), two, np.nextafter(two, m.dtype.type(3))]
    idx = rng.choice(d[t].size, 4 * 9, replace=False).reshape(4, 9)
    for rep in range(4):
        for j, (dv, mv) in enumerate((dv, mv) for dv in ds for mv in ms):
            d[t].flat[idx[rep, j]] = dv
            m[t].flat[idx[rep, j]] = mv


def specials(rng, m, t):
    """m of 0, -0, +inf, -inf, negative and -1e-8 (g = 1 / 0) in frame t."""
    vals = np.array([0.0, -0.0, np.inf, -np.inf, -1.0, -5.0, -1e-8], m.dtype)
    idx = rng.choice(m[t].size, 3 * vals.size, replace=False)
    m[t].flat[idx] = np.tile(vals, 3)


def case_even(rng):
    d, m = frames(rng, 4, 24, 32, np.float32)
    for t in range(4):
        boundaries(rng, d, m, t)
    d[2][rng.random(d[2].shape) < 0.6] = rng.uniform(0.0, 0.0099, 1).astype(np.float32)   # sky: more than half below 0.01
    specials(rng, m, 3)
    return d, m, (48, 64)


def case_odd(rng):
    d, m = frames(rng, 3, 23, 31, np.float32)
    boundaries(rng, d, m, 0)
    specials(rng, m, 1)
    return d, m, (23, 31)


def case_f64(rng):
    d, m = frames(rng, 3, 24, 32, np.float64)
    boundaries(rng, d, m, 1)
    specials(rng, m, 2)
    return d, m, (24, 32)


def case_odd_f64(rng):
    d, m = frames(rng, 2, 23, 31, np.float64)
    boundaries(rng, d, m, 0)
    return d, m, (46, 62)


def case_single(rng):
    d, m = frames(rng, 1, 24, 32, np.float32)
    boundaries(rng, d, m, 0)
    return d, m, (24, 32)


def case_ties(rng):
    d, m = frames(rng, 3, 24, 32, np.float32)
    d = (np.round(d * 8) / 8 + 0.01).astype(np.float32)                   # 9 distinct disparities
    m = np.round(m).astype(np.float32) + 0.5                               # whole metres and a half
    d[2], m[2] = d[1], m[1]                                                # p_1 == p_2 == median(p): argmin meets a tie
    return d, m, (24, 32)


def case_nan_metric(rng):
    d, m = frames(rng, 3, 23, 31, np.float32)
    m[1].flat[rng.choice(m[1].size, 5, replace=False)] = np.nan
    return d, m, (23, 31)


def case_nan_mono(rng):
    d, m = frames(rng, 2, 24, 32, np.float32)
    d[1].flat[rng.choice(d[1].size, 3, replace=False)] = np.nan
    return d, m, (24, 32)


def case_mismatch(rng):
    d, m = frames(rng, 5, 24, 32, np.float32)
    return d, m[:4], (24, 32)


CASES = {"even": case_even, "odd": case_odd, "f64": case_f64, "odd_f64": case_odd_f64, "single": case_single, "ties": case_ties,
         "nan_metric": case_nan_metric, "nan_mono": case_nan_mono, "mismatch": case_mismatch}


def run_reference(root, case, d, m, intr, image_hw):
    from PIL import Image
    names = [f"{i:05d}" for i in range(max(len(d), len(m)))]
    mono_dir, metric_dir, img_dir = (os.path.join(root, x, case) for x in ("mono", "metric", "images"))
    for p in (mono_dir, metric_dir, img_dir):
        os.makedirs(p)
    for name, x in zip(names, d):
        np.save(os.path.join(mono_dir, name + ".npy"), x)
    for name, x, k in zip(names, m, intr):
        np.savez(os.path.join(metric_dir, name + ".npz"), depth=x, intrinsics=k)
    img = os.path.join(img_dir, "00000.png")
    Image.new("RGB", (image_hw[1], image_hw[0])).save(img)
    cv2.SIZES[img] = tuple(image_hw)
    out_d, out_k = os.path.join(root, "out", case), os.path.join(root, "out_K", case)
    with warnings.catch_warnings(), np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        ref.align_depth(os.path.join(root, "mono"), os.path.join(root, "metric"), case, img_dir, out_d, out_k)
    n = min(len(d), len(m))
    depth = np.stack([np.load(os.path.join(out_d, name + ".npy")) for name in names[:n]])
    Ks = [np.load(os.path.join(out_k, name + "_intrinsics.npy")) for name in names[:n]]
    assert all(np.array_equal(K, Ks[0]) for K in Ks) and sorted(os.listdir(out_d)) == [x + ".npy" for x in names[:n]]
    return names, depth, Ks[0]


def main():
    out = {}
    with tempfile.TemporaryDirectory() as root:
        for ci, (case, make) in enumerate(CASES.items()):
            rng = np.random.default_rng(300 + ci)
            d, m, image_hw = make(rng)
            H, W = m.shape[1:]
            fx = rng.uniform(0.8, 1.2, len(m)) * W
            intr = np.zeros((len(m), 3, 3), m.dtype)
            intr[:, 0, 0], intr[:, 1, 1], intr[:, 0, 2], intr[:, 1, 2], intr[:, 2, 2] = fx, fx, W / 2, H / 2, 1
            names, depth, K = run_reference(root, case, d, m, intr, image_hw)
            out.update({f"{case}.mono": d, f"{case}.metric": m, f"{case}.intrinsics": intr, f"{case}.image_hw": np.array(image_hw),
                        f"{case}.names": np.array(names), f"{case}.depth": depth, f"{case}.K": K})
            print(case, d.shape, m.dtype, "depth", depth.dtype, "finite", int(np.isfinite(depth).sum()), "of", depth.size)
    out["names"] = np.array(list(CASES))
    out["signatures"] = np.array(json.dumps({f: str(inspect.signature(getattr(ref, f)))
                                             for f in ("intrinsics_to_fov", "align_depth", "align_davis_demo")}))
    path = os.path.join(HERE, "mono_depth.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
