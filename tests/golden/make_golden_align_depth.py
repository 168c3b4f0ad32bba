#!/usr/bin/env python3
"""Golden vectors for align_depth_maps (main/global_refine/model/utils.py:268-312): runs the reference's UNMODIFIED function
on depth maps we generate, where the reference checkout is at hand (the pypose stand-in and the checkout on sys.path as for
make_golden_depth_eval.py).  Writes tests/golden/align_depth.npz, for every case `<case>.<dtype>.c<C>`:
  .maps      the input [T, 24, 32, C] (float32 or float64; a second channel holds its own values)
  .aligned   the reference's output (frame 0 whole; channel 0 only for the others, the np.zeros_like layout)
  .skipped   the frames the reference printed "Insufficient overlapping region" for, and .printed the counts it printed
Cases (each frame's positive set is drawn so that the overlap with its aligned predecessor is the count named):
  chain       T = 8: overlap 100 (even, exactly the threshold), 99 (skipped), then 301 right after the skipped frame (an
              even union of 99 + 301), heavy ties, +inf in the maps and in a median, NaN, zero, negative and -inf pixels
  empty_past  T = 3: no overlap at frame 1 (skipped), so frame 2's past set (A0 > 0) & (A1 > 0) is empty
  underflow   T = 4: s ~ 1e-300 (float64) / 1e-30 (float32) flushes part of frame 1 to 0 and part to subnormals; frame 2's
              overlap shrinks by the flushed pixels
  overflow    T = 7: s ~ 1e300 / 1e30 takes part of frame 1 to inf; then s = 0 (med_cur = inf), a skipped frame after an
              all-zero one, s = inf (med_prev = inf) and s = NaN (both inf), and a skipped frame after an all-NaN one
Only inputs we generated and the reference's outputs are written.

    python tests/golden/make_golden_align_depth.py
"""
import contextlib
import io
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/main/global_refine"
sys.path[:0] = [os.path.join(HERE, "refstubs"), REF]
from model.utils import align_depth_maps  # noqa: E402  (reference, unmodified)

H, W = 24, 32
HW = H * W
DTYPES = {"float32": np.float32, "float64": np.float64}


def frame(rng, pos, lo=0.5, hi=10.0, ties=None):
    """Channel 0 of one frame: positive on the index set `pos`, else a mix of 0, -0, negative values, -inf and NaN."""
    f = rng.choice(np.array([0.0, -0.0, -1.5, -np.inf, np.nan]), HW)
    f[pos] = rng.choice(ties, pos.size) if ties is not None else rng.uniform(lo, hi, pos.size)
    return f


def with_overlap(rng, prev_pos, n_overlap, n_other):
    """A positive set that meets `prev_pos` in exactly n_overlap pixels and holds n_other pixels outside it."""
    inside = rng.choice(prev_pos, n_overlap, replace=False)
    outside = rng.choice(np.setdiff1d(np.arange(HW), prev_pos), n_other, replace=False)
    return np.concatenate([inside, outside])


def chain(rng, dt):
    fs, P = [], []
    P.append(rng.choice(HW, 500, replace=False))
    f0 = frame(rng, P[0])
    f0[P[0][:3]] = np.inf                                          # +inf in the first median's set
    fs.append(f0)
    for n_ov, n_other, kw in ((100, 200, {}), (99, 300, {}), (301, 100, {}), (250, 150, {"ties": np.array([1.5, 2.5, 3.5])}),
                              (333, 0, {}), (200, 201, {"ties": np.array([0.75, 4.0])}), (400, 100, {"lo": 1e-3, "hi": 1e3})):
        P.append(with_overlap(rng, P[-1], n_ov, n_other))
        fs.append(frame(rng, P[-1], **kw))
    fs[5][P[5][:40]] = np.inf                                      # inf among the current set
    return np.stack(fs).astype(dt)


def empty_past(rng, dt):
    cols = np.arange(HW) % W
    f0 = frame(rng, np.flatnonzero(cols < 16))
    f1 = frame(rng, np.flatnonzero(cols >= 16))
    f2 = frame(rng, np.arange(HW))
    return np.stack([f0, f1, f2]).astype(dt)


def underflow(rng, dt):
    tiny, flush, sub = (1e-300, 1e-30, 1e-10) if dt == np.float64 else (1e-30, 1e-20, 1e-9)
    f0 = rng.uniform(0.5, 2.0, HW) * tiny
    f1 = rng.uniform(0.5, 2.0, HW)
    f1[:200] = rng.uniform(0.5, 2.0, 200) * flush                # s * these -> 0
    f1[200:260] = rng.uniform(0.5, 2.0, 60) * sub                 # s * these -> subnormal
    f2 = frame(rng, np.arange(HW))
    f3 = frame(rng, rng.choice(HW, 600, replace=False))
    return np.stack([f0, f1, f2, f3]).astype(dt)


def overflow(rng, dt):
    big = 1e300 if dt == np.float64 else 1e30
    f0 = rng.uniform(0.5, 2.0, HW) * big
    f1 = rng.uniform(0.5, 2.0, HW)
    f1[:200] *= 1e10                                               # s * these -> inf
    f2 = frame(rng, np.arange(HW))
    f2[:450] = np.inf                                              # med_cur = inf: s = 0, and 0 * inf = NaN
    f3 = frame(rng, np.arange(HW))                                 # (no overlap with a frame of zeros: skipped)
    f3[:500] = np.inf
    f4 = frame(rng, rng.choice(HW, 700, replace=False))            # med_prev = inf, med_cur finite: s = inf
    f5 = frame(rng, np.arange(HW))
    f5[:600] = np.inf                                              # med_prev = med_cur = inf: s = NaN
    f6 = frame(rng, np.arange(HW))                                 # (skipped after an all-NaN frame)
    return np.stack([f0, f1, f2, f3, f4, f5, f6]).astype(dt)


CASES = {"chain": (chain, (1, 2)), "empty_past": (empty_past, (1,)), "underflow": (underflow, (1, 2)), "overflow": (overflow, (1,))}


def main():
    out = {}
    names = []
    for ci, (case, (make, channels)) in enumerate(CASES.items()):
        for di, (dname, dt) in enumerate(DTYPES.items()):
            rng = np.random.default_rng(100 + 10 * ci + di)
            ch0 = make(rng, dt).reshape(-1, H, W)
            for C in channels:
                maps = np.zeros(ch0.shape + (C,), dt)
                maps[..., 0] = ch0
                if C > 1:
                    maps[..., 1:] = rng.uniform(-1.0, 5.0, maps[..., 1:].shape)
                buf = io.StringIO()
                with np.errstate(all="ignore"), contextlib.redirect_stdout(buf):
                    aligned = align_depth_maps(maps.copy())
                found = re.findall(r"between depth map (\d+) and (\d+) \((\d+) pixels\)", buf.getvalue())
                name = f"{case}.{dname}.c{C}"
                names.append(name)
                out[f"{name}.maps"] = maps
                out[f"{name}.aligned"] = aligned
                out[f"{name}.skipped"] = np.array([int(b) for _, b, _ in found], np.int64)
                out[f"{name}.printed"] = np.array([int(c) for _, _, c in found], np.int64)
                print(name, "skipped", out[f"{name}.skipped"].tolist(), "counts", out[f"{name}.printed"].tolist())
    out["names"] = np.array(names)
    path = os.path.join(HERE, "align_depth.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
