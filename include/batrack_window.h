/* batrack_window.h — C ABI of the tracker's window preparation (the reference's main/frontend/md_tracker.py:416-671,
 * `MDTracker.forward`): the depth range of the video, the window's normalised depth maps and their range, the 3-D feature
 * maps (`embedConv` over the encoder's maps and a Fourier embedding of (x, y, z) that is never in memory), and the features
 * of new tracks sampled from their own frames.  The encoder `fnet` is not here.
 *
 * Inference only, float32, B = 1.  C = BT_WINDOW_C = 128 feature channels, BT_WINDOW_EMB = 63 embedding channels.
 *
 * depth_process(d) = d, or logf(max(d, 1e-3)) when use_log_depth (a NaN stays NaN).
 *
 * bt_depth_range.  out[0] = min, out[1] = max of depth_process(d) over the T frames of `depth` (element (t, y, x) at
 * t * stride_t + y * stride_y + x * stride_x: the channel view rgbds[0, :, 3] is read in place), over the elements with
 * d > 0.01 when use_log_depth == 0 (md_tracker.py:438-443), over all of them otherwise.  No element selected: out =
 * (+inf, -inf).  The mask never selects a NaN; with use_log_depth a NaN makes both results NaN, as torch's min() and
 * max() do.  One launch; the blocks leave their partial results in
 * `workspace` and the last one to finish reduces them.
 *
 * bt_window_depth.  For the S frames of a window whose first `frames` (1 <= frames <= S) are at `depth` (frame t >= frames
 * is frame frames - 1 again: the padding of a short last window, md_tracker.py:502-506):
 *   dmaps[t, y, x] = ((depth_process(d[t, y * stride, x * stride]) - d_near) / d_range) * Dz,   h = H / stride, w = W / stride,
 * every operation rounded, the division the correctly rounded one: bit-equal to md_tracker.py:513-517 in float32 where
 * F.interpolate(scale_factor = 1 / stride, mode = "nearest") is the slice [::stride, ::stride] (stride a power of two).
 * d_range is float32(d_far - d_near), the difference taken in double as the reference's Python floats do.
 * zrange[0] = min, zrange[1] = max of dmaps over ALL S frames, in the same launch (a NaN makes both NaN, as torch's do).
 *
 * workspace (both): bt_window_workspace_bytes() bytes, whose LAST 4 bytes are zero on entry (a ticket; the kernel leaves it
 * zero again).  Two calls in flight must not share one.
 *
 * bt_embed_conv.  out[f, o, y, x] = bias[o] + sum over taps (ky, kx) in 3 x 3 and channels c < 191 of
 *   W[o, c, ky, kx] * in[f, c, y + ky - 1, x + kx - 1],   a tap outside the map contributing 0 for every c (zero padding);
 *   in[f, c] for c < 128: fnet[f, c, :, :], element at f * sf + c * sc + y * sy + x * sx (any layout, read in place);
 *   in[f, 128 + e]: the embedding of p = (px, py, pz), px = 2 ((x - 0) / ((w - 1) - 0) - 0.5), py likewise with y and h,
 *     pz = 2 ((z - zrange[0]) / (zrange[1] - zrange[0]) - 0.5) with z = dmaps[frame0 + f, y, x]; every operation rounded;
 *     e < 3: p[e];  e = 3 + 6 i + r: r < 3: sin(p[r] * freqs[i]), else cos(p[r - 3] * freqs[i]), the product one float32
 *     multiply, sine and cosine with full argument reduction (the arguments reach 1024 rad)  — Embedder_Fourier's order.
 * `wpacked` is W repacked as [24][9][8][128]: wpacked[c / 8][3 ky + kx][c % 8][o] = W[o][c][ky][kx], zero for c = 191.
 * Summed on v_mfma_f32_16x16x4_f32 in the kernel's own fixed order (channel chunks of 8, then taps, then groups of 4
 * channels; csrc/window_fmaps.hip), the bias added last: a call repeats bit for bit, and a frame's result does not depend
 * on frame0 or F.  dmaps is [S, h, w] and zrange the pair of bt_window_depth, both read on the device; out is [F, 128, h, w]
 * contiguous (a slice of the window's buffer).  zrange[0] == zrange[1] makes every output NaN, as in the reference.
 *
 * bt_feat_sample.  out[k, c] = bilinear_sample2d(fmaps[clamp(frames[k], 0, S - 1), c]) at (x, y) = xy[k * xy_stride + 0 .. 1]
 * (frontend/core/model_utils.py:75-158: floor, corner indices clamped to the map, weights from the unclamped corners, every
 * product rounded, the four summed left to right; the floor of a coordinate that does not fit an int32 is INT_MIN, as on
 * the reference's x86 host).  fmaps [S, C, h, w] contiguous.  Bit-equal to md_tracker.py:567-575 in float32.
 *
 * All pointers are DEVICE pointers; `stream` is a hipStream_t as void*.  Returns
 *   BT_EINVAL        a null pointer, a non-positive size, frames outside 1 .. S, frame0 < 0 or frame0 + F > S, stride < 1,
 *                    H / stride or W / stride < 1, xy_stride < 2, n < 0, h or w < 2 (bt_embed_conv: the x and y ranges
 *                    would be 0 / 0);
 *   BT_EUNSUPPORTED  C != 128, or a size, a stride or an element count above 2^31 - 1;
 *   BT_OK            otherwise — with nothing launched for n == 0 or F == 0;   BT_EHIP if a launch fails.
 * Every refusal happens before anything is launched. */
#ifndef BATRACK_WINDOW_H
#define BATRACK_WINDOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BT_WINDOW_C 128
#define BT_WINDOW_EMB 63
#define BT_WINDOW_FREQS 10
#define BT_WINDOW_KCHUNK 8       /* input channels per K-chunk of bt_embed_conv: wpacked is [192 / 8][9][8][128] */

size_t bt_window_workspace_bytes(void);

int bt_depth_range(const float *depth, int64_t T, int64_t H, int64_t W, int64_t stride_t, int64_t stride_y, int64_t stride_x,
                   int32_t use_log_depth, void *workspace, float *out, void *stream);

int bt_window_depth(const float *depth, int64_t frames, int64_t S, int64_t H, int64_t W, int64_t stride_t, int64_t stride_y,
                    int64_t stride_x, int64_t stride, float d_near, float d_range, float Dz, int32_t use_log_depth,
                    void *workspace, float *dmaps, float *zrange, void *stream);

int bt_embed_conv(const float *fnet, int64_t sf, int64_t sc, int64_t sy, int64_t sx, const float *dmaps, const float *zrange,
                  const float *wpacked, const float *bias, const float *freqs, int64_t S, int64_t frame0, int64_t F,
                  int64_t h, int64_t w, int64_t C, float *out, void *stream);

int bt_feat_sample(const float *fmaps, int64_t S, int64_t C, int64_t h, int64_t w, const int32_t *frames, const float *xy,
                   int64_t xy_stride, int64_t n, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_WINDOW_H */
