"""The reference's align_depth_maps (main/global_refine/model/utils.py:268-312) restated with its branch decisions exposed: the
aligned channel 0 and, per frame, what bt_align_depth_maps reports (include/batrack_depth.h) — `scales` (s widened to float64,
NaN for frame 0 and skipped frames), `overlap` (c, 0 for frame 0) — plus the size of the union med_prev is taken over."""
import numpy as np


def host_align_stats(ch0):
    ch0 = np.asarray(ch0)
    T = ch0.shape[0]
    out = np.zeros_like(ch0)
    out[0] = ch0[0]
    scales, overlap, union = np.full(T, np.nan), np.zeros(T, np.int64), np.zeros(T, np.int64)
    with np.errstate(all="ignore"):
        for i in range(1, T):
            prev, cur = out[i - 1], ch0[i]
            mask = (prev > 0) & (cur > 0)
            overlap[i] = mask.sum()
            if overlap[i] < 100:
                out[i] = cur
                continue
            if i == 1:
                pv = prev[mask]
            else:
                past = out[i - 2]
                pv = np.concatenate((past[(past > 0) & (prev > 0)], prev[mask]))
            union[i] = pv.size
            s = np.median(pv) / np.median(cur[mask])
            scales[i] = float(s)
            out[i] = s * cur
    return out, scales, overlap, union
