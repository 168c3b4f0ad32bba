/* batrack_video.h — C ABI of the tracker's input preparation (csrc/video_prep.hip): what the reference's
 * `BATRACK._compute_sparse_tracks` (main/batrack.py:529-587) and the head of `MDTracker.forward`
 * (main/frontend/md_tracker.py:435-443) do to the frames of the local window before the encoder sees them — the bilinear
 * resize of colour and depth to the tracker's size, the colour mapping to [-1, 1], and the masked range of the resized depth.
 * One launch for F frames; a frame's result depends on that frame alone, whatever F is.
 *
 * Inference only, float32 out.  Conventions of batrack_ba.h: DEVICE pointers, `stream` is a hipStream_t passed as void*,
 * integer status codes, every argument check returns before anything is enqueued, nothing allocates or synchronises.
 *
 * Inputs.  image: F frames of 3 channels of H x W, uint8 (image_is_u8 != 0) or float32, element (f, c, y, x) at
 * f * si_f + c * si_c + y * si_y + x * si_x with the strides in ELEMENTS: a planar [F, 3, H, W] array and the permuted view of
 * an [F, H, W, 3] one are both read as they lie.  depth: float32, element (f, y, x) at f * sd_f + y * sd_y + x * sd_x.
 * Neither is written.
 *
 * Resize.  rgbd[f, c] (c = 0 .. 2 the colours, c = 3 the depth) is the bilinear resize of plane c to oh x ow as
 * F.interpolate(mode="bilinear", align_corners=False, antialias=False) defines it, with the source coordinate taken EXACTLY.
 * The source row of output row oy is max(0, (oy + 0.5) * H / oh - 0.5); in integers
 *     num = max(0, (2 oy + 1) * H - oh),   den = 2 oh,   y0 = num div den,   ly1 = float(num mod den) / float(den),
 *     ly0 = 1 - ly1,   y1 = y0 + (y0 < H - 1 ? 1 : 0),
 * the quotient ly1 rounded once (both integers are exact in float32 while den < 2^24; only for an output side of 2^23 or more
 * is the quotient taken in float64 and rounded to float32, which rounds twice).  Columns alike with ox, W, ow.  With a, b the taps (y0, x0), (y0, x1) and c, d the taps
 * (y1, x0), (y1, x1), converted to float32 exactly when uint8,
 *     v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d),
 * every product and sum rounded on its own (no contraction).  All four taps are multiplied even at weight 0, so a NaN or an
 * infinity reaches every pixel that has it among its taps, and no other.  With oh == H and ow == W every ly1 and lx1 is 0
 * and v == a bit for bit for every finite a other than -0.
 * (torch computes the coordinate in float32: at 436 x 1024 -> 384 x 512 that alone moves its float32 result 5e-3, on values
 * up to 255, away from its float64 result.  The exact coordinate is the float64 result's.)
 *
 * Normalisation.  With normalise != 0 planes 0 .. 2 are stored as 2 * (v / 255.0f) - 1, the division the correctly rounded
 * one, each operation rounded: md_tracker.py:435 in float32 as a CPU run computes it.  Plane 3 is never changed.
 *
 * Depth range.  drange[f] = (min, max) of depth_process(d) over the oh x ow values d of rgbd[f, 3], with the rules of
 * bt_depth_range (include/batrack_window.h): over the d > 0.01 when use_log_depth == 0, over all of them otherwise; nothing
 * selected gives (+inf, -inf); the mask never selects a NaN, and with use_log_depth a NaN makes both NaN.  Bit-equal to
 * bt_depth_range run on the plane rgbd[f, 3].  Taken in the same launch from the values just written, by the reduction of
 * csrc/minmax_reduce.hpp: per frame, one (min, max) pair per block in the workspace and a ticket.
 *
 * workspace: bt_frame_prep_workspace_bytes(F, oh, ow) bytes.  Its FIRST F 32-bit words are the frames'
 * tickets: zero on entry, and left zero.  The rest (the blocks' pairs, from byte 16 * ceil(F / 4)) needs no initialisation.
 * So calls with the same ceil(F / 4) may reuse one workspace without zeroing it again; a call with another F finds the pairs of
 * the last one where its tickets are, and needs them zeroed.  Two calls in flight must not share one.  The size is 0 when a size is not positive or the call would be refused as
 * unsupported.
 *
 * rgbd [F, 4, oh, ow] float32 contiguous; stored 16 bytes a lane when ow is a multiple of BT_VIDEO_VEC and rgbd is 16-byte
 * aligned, element by element otherwise (the same values).  drange [F, 2].  Neither may overlap an input.
 *
 * Returns
 *   BT_EINVAL        a null image, depth, workspace, rgbd or drange; F < 0; H, W, oh or ow < 1; a negative stride;
 *   BT_EUNSUPPORTED  F, H, W, oh, ow, a stride, an input's element count or farthest element offset, or
 *                    F * 4 * oh * ow, above 2^31 - 1;
 *   BT_OK            otherwise — with nothing launched for F == 0;   BT_EHIP if the launch fails.
 * Every refusal happens before anything is launched. */
#ifndef BATRACK_VIDEO_H
#define BATRACK_VIDEO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BT_VIDEO_VEC 4            /* output columns a lane: one 16-byte store per plane */
#define BT_VIDEO_TILE 1024        /* output pixels a block covers per trip: 256 lanes of BT_VIDEO_VEC columns */
#define BT_VIDEO_MAX_BLOCKS 1024  /* blocks per frame at the most: larger frames take several trips */
#define BT_VIDEO_GRID_FRAMES 64   /* the grid's frame dimension at the most: more frames take several trips */

size_t bt_frame_prep_workspace_bytes(int64_t F, int64_t oh, int64_t ow);

int bt_frame_prep(const void *image, int32_t image_is_u8, int64_t si_f, int64_t si_c, int64_t si_y, int64_t si_x,
                  const float *depth, int64_t sd_f, int64_t sd_y, int64_t sd_x,
                  int64_t F, int64_t H, int64_t W, int64_t oh, int64_t ow,
                  int32_t normalise, int32_t use_log_depth,
                  void *workspace, float *rgbd, float *drange, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_VIDEO_H */
