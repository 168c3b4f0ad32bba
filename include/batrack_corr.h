/* batrack_corr.h — C ABI of the tracker's correlation lookup, fused: `CorrBlock.corr` + `CorrBlock.sample`
 * (the reference's main/frontend/core/cotracker/blocks.py:326-385, called per refinement iteration by
 * main/frontend/md_tracker.py:250-252,344-346) without the correlation volume.
 *
 * Specification.  fmaps [S', C, H, W] float32 (S' = B * S frames); levels l = 0 .. L-1, radius r, d = 2r + 1.
 *   Pyramid:  F_0 = fmaps;  F_{l+1} = the 2 x 2 mean of F_l at stride 2, H_{l+1} = floor(H_l / 2), W_{l+1} = floor(W_l / 2)
 *             (an odd last row / column is dropped: 45 x 61 -> 22 x 30).
 *   Volume (never formed):  D_l[s, n, y, x] = <targets[s, n, :], F_l[s, :, y, x]> / sqrt(float32(C)) for integer (y, x)
 *             inside level l's map, and 0 outside it.
 *   Lookup:   (cx, cy) = coords[s, n] / 2^l,  x0 = floor(cx), fx = cx - x0,  y0 = floor(cy), fy = cy - y0;  for a, b in [0, d):
 *               out[s, n, l*d*d + a*d + b] = (1-fx)(1-fy) D_l[Y, X] + fx (1-fy) D_l[Y, X+1] + (1-fx) fy D_l[Y+1, X] + fx fy D_l[Y+1, X+1]
 *               with X = x0 - r + a,  Y = y0 - r + b
 *             — the bilinear sample of D_l at x = cx - r + a, y = cy - r + b.  NOTE THE ORDER: the FIRST window index a
 *             moves x, the second, b, moves y (the reference adds a (dy, dx) mesh onto (x, y) coordinates).
 *             A tap outside the map contributes exactly 0 and its feature row is not read; a tap inside the map is
 *             multiplied by its weight even where that weight is 0 (a NaN feature row shows wherever the reference's
 *             grid_sample would show it, and nowhere else).
 *             Coordinates may be any float.  The integer part is clamped far outside every map before the positions are
 *             formed, so a finite coordinate however far away (+-3e9, +-(1e6 +- 0.5), 2^24 + 1) gives exactly 0.  A
 *             coordinate that is +-inf or NaN has a NaN fraction: every output of its query is NaN, at every level, and
 *             no other query is touched — what the volume formulation gives (tests/test_gpu_corr_limits.py).
 *
 * bt_corr_pyramid writes all L levels CHANNELS-LAST into one packed buffer: level l is [S', H_l, W_l, C] float32 and
 * starts at float offset  C * S' * sum_{k<l} H_k W_k;  bt_corr_pyramid_bytes gives the buffer's size (0 for arguments
 * bt_corr_pyramid would refuse).  One call per CorrBlock; the lookups read only this buffer.
 *
 * bt_corr_lookup: targets [S', N, C] float32 contiguous; coords: N * S' (x, y) pairs in level-0 pixels, pair k at
 * coords + k * coord_stride floats (coord_stride >= 2: 2 for a contiguous [S', N, 2] tensor, 3 for the tracker's
 * `coords[..., :2]` view of a [S', N, 3] tensor); out [S', N, L*d*d] float32 contiguous, every element written.
 * float32 accumulation with fused multiply-adds in a fixed order, no atomics, no workspace: a call repeats bit for bit.
 * Summation order of a dot product over the C channels, per kernel (csrc/corr_lookup.hip): the generic kernel, 16 lanes
 * each with one chain of 4 * ceil(C / 64) fused multiply-adds, then added pairwise across the lanes; lanes across channels
 * (C = 128), 32 lanes x a chain of 4, added pairwise; lane = position (C = 128), 16 interleaved chains of 8 in one lane,
 * added pairwise.  Measured, not guaranteed: at the shapes of tests/test_gpu_corr_limits.py every kernel stays within twice
 * the float32 rounding error of the formulas above evaluated in numpy.
 *
 * All pointers are DEVICE pointers; `stream` is a hipStream_t as void*.  Returns
 *   BT_EINVAL        a null pointer, a non-positive size, C not a multiple of 4, levels < 1, radius < 0, coord_stride < 2,
 *                    or a map too small for its pyramid (min(H, W) >> (levels - 1) == 0);
 *   BT_EUNSUPPORTED  C > 512, radius > 7, levels > 8, H or W > 32768, S * N * levels > 2^31 - 1;
 *   BT_OK            otherwise — with nothing launched for N == 0;   BT_EHIP if a launch fails.
 * Every refusal happens before anything is launched. */
#ifndef BATRACK_CORR_H
#define BATRACK_CORR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BT_CORR_MAX_LEVELS 8
#define BT_CORR_MAX_RADIUS 7
#define BT_CORR_MAX_CHANNELS 512

size_t bt_corr_pyramid_bytes(int64_t S, int64_t C, int64_t H, int64_t W, int32_t levels);

int bt_corr_pyramid(const float *fmaps, int64_t S, int64_t C, int64_t H, int64_t W, int32_t levels,
                    float *pyramid, void *stream);

int bt_corr_lookup(const float *pyramid, int64_t S, int64_t C, int64_t H, int64_t W, int32_t levels, int32_t radius,
                   const float *targets, const float *coords, int64_t coord_stride, int64_t N,
                   float *out, void *stream);

/* Measurement only: which lane layout the C = 128, r = 3 lookup uses.  0 (the default): lanes across channels;
 * 1: one lane per window position;  2: the generic kernel.  Returns the previous value; any other argument only reads it. */
int bt_config_corr_lookup_layout(int32_t layout);

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_CORR_H */
