/* batrack_depth.h — C ABI of the video-depth metrics the reference reports after its dense global alignment, and of the
 * depth-map alignment that prepares that stage.
 *
 * Reference: main/global_refine/model/utils.py:103-116 (eval_depth), :187-201 (align_with_lstsq), :203-240
 * (compute_errors), :253-265 (eval_depth_metric), :268-312 (align_depth_maps), and main/mono_depth/get_mono_depth.py:21-150
 * (align_depth: mono disparity to metric depth, bt_mono_align).  The reference scores a refined depth map
 * against ground truth in numpy on the host; bt_depth_metrics does the same for one pair of arrays on the device, and
 * bt_align_depth_maps aligns a scene's depth maps there.  Device pointers, sizes, integer status codes
 * (include/batrack_ba.h); nothing allocates or synchronises.
 */
#ifndef BATRACK_DEPTH_H
#define BATRACK_DEPTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BT_DEPTH_SCALE_NONE 0
#define BT_DEPTH_SCALE_MEDIAN 1
#define BT_DEPTH_SCALE_LSTSQ 2

/* Bytes of device workspace bt_depth_metrics needs for n elements (independent of the data); BT_EINVAL for n < 0,
 * BT_EUNSUPPORTED for n > 2^31 - 1. */
int64_t bt_depth_metrics_workspace_bytes(int64_t n);

/* compute_errors(gt[valid], pred[valid], depth_min, depth_max, scaling) for the valid set
 *   valid = mask & (gt > depth_min) & (gt < depth_max)          (mask NULL: every element; a nonzero byte is true)
 * scaling BT_DEPTH_SCALE_MEDIAN: pred *= median(gt_v) / median(pred_v), numpy's median (exact selection; an even count takes
 *   the float64 mean of the two middle elements) by radix select on the order-preserving key of the float32 values;
 * BT_DEPTH_SCALE_LSTSQ: pred = s pred + t, (s, t) the least-squares fit of gt by [pred, 1] from the count, the means and the
 *   centred second moments Cpp = sum (p - mean p)^2, Cpg = sum (p - mean p)(g - mean g) in float64 (merged pairwise in a fixed
 *   order): s = Cpg / Cpp, t = mean g - s mean p, so a pred of small relative spread loses nothing to cancellation; a singular
 *   system (in np.linalg.lstsq's sense, sigma_min <= rcond sigma_max with rcond = eps * max(count, 2), decided from
 *   det = count Cpp) gets the minimum-norm solution;
 * BT_DEPTH_SCALE_NONE: no scaling.
 * Then pred is clamped to [depth_min, depth_max] and every per-element operation runs in float64 on the float32 inputs.
 * out [11] (device, float64): abs_rel, sq_rel, log10, rmse, rmse_log, a1, a2, a3 (the reference's order), then the valid count,
 * the ratio (median) or s (lstsq) or 1, and t (lstsq) or 0.  An empty valid set gives NaN for the eight metrics (BT_OK); a NaN
 * among the valid preds propagates as numpy propagates it.  Sums are per-workgroup float64 partials reduced in a fixed order:
 * a call is bit-for-bit repeatable.  The median's key takes -0 and +0 for one value and decodes it as +0, where numpy returns
 * whichever zero sits in the middle: the sign of a median that is zero is not pinned.  `workspace`:
 * bt_depth_metrics_workspace_bytes(n) bytes, 16-byte aligned (BT_EINVAL otherwise), contents arbitrary.  n > 2^31 - 1:
 * BT_EUNSUPPORTED, checked before anything is enqueued.  Enqueued on `stream`. */
int bt_depth_metrics(const float *gt, const float *pred, const uint8_t *mask, int64_t n, float depth_min, float depth_max,
                     int32_t scaling, void *workspace, double *out, void *stream);

#define BT_DEPTH_F32 0
#define BT_DEPTH_F64 1

/* Bytes of device workspace bt_align_depth_maps needs for frames of hw pixels (independent of the data and of T); BT_EINVAL
 * for hw < 1 or a bad dtype, BT_EUNSUPPORTED for hw >= 2^30. */
int64_t bt_align_depth_maps_workspace_bytes(int64_t hw, int32_t dtype);

/* align_depth_maps (main/global_refine/model/utils.py:268-312) on channel 0 of T depth maps of hw pixels, in the dtype
 * (BT_DEPTH_F32: float, BT_DEPTH_F64: double) as numpy computes it.  aligned[0] = maps[0]; then for i = 1 .. T-1 in order
 *   m = (aligned[i-1] > 0) & (maps[i] > 0),  c = count(m)
 *   c < 100:  aligned[i] = maps[i]
 *   else:     aligned[i] = s * maps[i],  s = med_prev / med_cur (one correctly rounded division in the dtype),
 *             med_cur = median(maps[i][m]),  med_prev = median(aligned[0][m]) for i == 1, else the median of the multiset
 *             aligned[i-2][(aligned[i-2] > 0) & (aligned[i-1] > 0)] + aligned[i-1][m]
 * with numpy's median (exact selection; an even count takes np.mean of the two middle elements in the dtype).  The `> 0`
 * tests drop NaN; every pixel is scaled, NaN and non-positive ones included.  The frames are a chain: each reads the
 * materialised aligned[i-1] and aligned[i-2].  `maps`, `aligned`: device, [T, hw] contiguous, the same buffer (in place) or
 * not overlapping.  scales [T] (device float64, or NULL): s widened, NaN for frame 0 and skipped frames.  overlap [T] (device
 * int64, or NULL): c, 0 for frame 0.  The whole chain is one fixed sequence of launches on `stream`: the counts, the branch,
 * the medians and s stay in device state (integer atomics only: a call repeats bit for bit).  `workspace`:
 * bt_align_depth_maps_workspace_bytes(hw, dtype) bytes, 16-byte aligned, contents arbitrary.  BT_EINVAL for T < 1, hw < 1, a
 * bad dtype, a NULL maps / aligned / workspace or a partial overlap of the two buffers; BT_EUNSUPPORTED for hw >= 2^30 (a union
 * count, at most 2 hw, stays below 2^31); both before anything is enqueued. */
int bt_align_depth_maps(const void *maps, void *aligned, int64_t T, int64_t hw, int32_t dtype, double *scales, int64_t *overlap,
                        void *workspace, void *stream);

/* Bytes of device workspace bt_mono_align needs for T frames of hw pixels (independent of the data; it grows with T, about
 * 4.2 KB a frame); BT_EINVAL for T < 1, hw < 1 or a bad dtype, BT_EUNSUPPORTED for T * hw > 2^31 - 1. */
int64_t bt_mono_align_workspace_bytes(int64_t T, int64_t hw, int32_t dtype);

/* align_depth (main/mono_depth/get_mono_depth.py:21-150) on T frames of hw pixels: relative mono disparity `mono` (float32) to
 * metric depth, given the metric depth `metric` of the same frames in the dtype D (BT_DEPTH_F32: float, BT_DEPTH_F64: double),
 * as numpy computes it in D.  Per frame t (d = mono[t], m = metric[t])
 *   g = 1 / (m + 1e-8);  g = 1e-2 where (m < 2) & (d < 0.02)            (d < 0.02 in float32)
 *   s_t = median((g - median(g) + 1e-8) / (d - median(d) + 1e-8)),  c_t = median(g - s_t d)
 * (median(d) and d - median(d) + 1e-8 in float32, the rest in D); then across the scene
 *   p = s c,  k = argmin |p - median(p)|  (the first index on ties; the first NaN if any, so k = 0 when median(p) is NaN)
 *   a_s = s_k,  a_c = c_k,  n = percentile(a_s d + a_c over all T * hw elements, 98) / 2
 *   depth_out = clip(1 / ((1 / n) (a_s d + a_c)), 1e-4, 1e4),  0 where that is below 1e-2
 * with numpy's median (exact selection; an even count takes np.mean of the two middle elements in the dtype) and numpy's
 * 'linear' percentile (q = D(98) / D(100), the index (T hw - 1) q, its floor, the next index and gamma in D, and np.lerp's two
 * forms either side of gamma = 0.5); a NaN in a median's or the percentile's input makes it NaN.  Every operation is rounded once
 * in D (no fused multiply-add) and divisions are correctly rounded.
 * `mono` [T, hw] float32, `metric` [T, hw] D, `depth_out` [T, hw] D: device, contiguous.  Optional (NULL: not written), in D:
 * frame_scale [T] (s), frame_shift [T] (c), aligns [3] (a_s, a_c, n); med_index [1] int64 (k).  The whole computation is one fixed
 * sequence of launches on `stream`: the medians, k and n stay in device state (integer atomics only: a call repeats bit for bit).
 * The optional outputs are independent: any of the 16 patterns of NULL gives the same depth_out and the same values in the
 * outputs that are present.  mono, metric and depth_out need their element's alignment only: 16-byte aligned pointers (with
 * hw % 4 == 0 for the per-frame passes) take 16-byte loads and stores, any other the scalar kernels, with the same bits.  The
 * call reads mono and metric and writes nothing but the outputs' own elements and the workspace.
 * `workspace`: bt_mono_align_workspace_bytes(T, hw, dtype) bytes, 16-byte aligned, contents arbitrary (what an earlier call left,
 * of this or another T, included: every call clears what it reads).  BT_EINVAL for T < 1,
 * hw < 1, a bad dtype, a NULL mono / metric / depth_out / workspace, a pointer not aligned to its element, or an output or the
 * workspace that overlaps an input (or the workspace an output); BT_EUNSUPPORTED for T * hw > 2^31 - 1; both before anything is
 * enqueued. */
int bt_mono_align(const float *mono, const void *metric, int64_t T, int64_t hw, int32_t dtype, void *depth_out, void *frame_scale,
                  void *frame_shift, void *aligns, int64_t *med_index, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_DEPTH_H */
