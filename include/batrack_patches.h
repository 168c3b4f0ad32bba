/* batrack_patches.h — the first step of a frame of the reference's BATRACK.__call__, on the device (csrc/patch_gen.hip):
 * `generate_patches(image)` (main/batrack.py:230-325) in the mode `PATCH_GEN: grid_grad_<G>`, `init_depth(patches, depth,
 * mode='dmap')` (:917-934) and the colour row of `colors_` (:978-979).  Two entries, one launch each:
 *     bt_image_gradient    the pooled gradient-magnitude map g of the image (`__image_gradient_2`, :214-221)
 *     bt_patch_generate    candidates, their scores on g, the per-cell selection, and the selected patches' rows
 * g is an INPUT of the second entry, so a caller (a test) may hand it any map of the right size.
 * No atomics: a call repeats bit for bit.  Every float32 operation below is rounded on its own (no contraction), division
 * and square root are the correctly rounded ones.
 *
 * Conventions of batrack_ba.h: DEVICE pointers, `stream` is a hipStream_t passed as void*, integer status codes, every
 * argument check returns before anything is enqueued, nothing allocates or synchronises.
 *
 * Inputs.  image: 3 channels of H x W, uint8 (BT_IMAGE_U8) or float32 (BT_IMAGE_F32), addressed as
 * image[c*stride_c + y*stride_y + x*stride_x] with the three strides in ELEMENTS, so that both a planar [3,H,W] array and
 * the permuted view of an [H,W,3] one are taken as they lie.  depth [H,W] float32, contiguous.  G >= 1 cells a side,
 * gm >= 1 patches a cell.  ux, uy [G*G, 8*gm] float32: the two uniform draws of :291-292, in that order.
 *     M = G*G*gm,  C = 8*gm,  W_grid = W div G,  H_grid = H div G,  cell c = cy*G + cx.
 *
 * (a) The map g [Hp, Wp], Hp = (H+1) div 4, Wp = (W+1) div 4.  With s(y,x) the sum of the three channels, 0 outside the
 * image, on the (H+1) x (W+1) lattice of the zero-padded image (:215-218)
 *     dx = s(y-1,x) - s(y-1,x-1),   dy = s(y,x-1) - s(y-1,x-1),   v = sqrt(dx*dx + dy*dy)      float32, correctly rounded
 *     g[i,j] = (sum of v[4i+a, 4j+b], a = 0..3 outer, b = 0..3 inner, added in float32 in that order) * 0.0625f
 * uint8 input: integers up to the root (dx*dx + dy*dy <= 1,170,450 < 2^24 is exact in float32).  float32 input:
 * s = (c0 + c1) + c2, products and sums rounded one by one; bit-pinned only for integer-valued images.
 *
 * (b) Candidates, i in [0, C) of cell c:
 *     x  = ux*0.7f + 0.15f                  xg = x*(float)W_grid + (float)(cx*W_grid)        yg alike with H_grid, cy
 *     rx = rintf(xg)                        x_norm = rx / (float)(W-1) * 2 - 1
 *     BT_PATCH_ROWS_REFERENCE:  y_norm = x_norm / (float)(H-1) * 2 - 1     (what :307-309 compute: coords_norm aliases coords)
 *     BT_PATCH_ROWS_IMAGE:      y_norm = rintf(yg) / (float)(H-1) * 2 - 1  (the evident intent)
 * score = the bilinear sample of g at (x_norm, y_norm), align-corners, zero padding (F.grid_sample, :311):
 *     ix = ((x_norm+1)/2)*(Wp-1), iy alike; taps nw, ne, sw, se with the weights (x1-ix)(y1-iy), (ix-x0)(y1-iy),
 *     (x1-ix)(iy-y0), (ix-x0)(iy-y0); a tap outside the map is skipped, a tap inside is multiplied even at weight 0.
 * The score's last bits are not pinned (torch's own CPU and GPU kernels differ there).
 *
 * (c) Selection.  The candidates of a cell are ranked ascending by (score, i), a NaN above every number, -0 equal to +0:
 * torch.argsort(stable=True).  Output slot r in [0, gm) of cell c takes the candidate of rank C - gm + r:
 *     sel[c*gm + r] = its i;     coords[c*gm + r] = its (xg, yg), unrounded.
 * (gm = 1 is the reference; gm > 1, where the reference raises, is its natural extension.)
 *
 * (d) The patch row p = c*gm + r.
 *     (px, py)  the correlation.py:55-66 blend (radius 0) of the coordinate grid at coords[p]: the grid's x plane holds j
 *               and its y plane i at pixel (i, j), 0 outside the image; the grid is never materialised
 *     clr[p]    the same blend of the three image channels, as float32, at coords[p] + 0.5f
 *     colors[p] (uint8)clr[p], by truncation
 *     d         bilinear_sample2d (model_utils.py:75-158: clamped indices, left-to-right sum) of depth at (px, py)
 *     patches[p] = (px, py, 1 / (d < 1e-2f ? 1e-2f : d))              a NaN d stays NaN
 * Inputs are never written.  clr, colors, coords, sel may each be NULL: not written then.
 *
 * Return codes.  bt_image_gradient: BT_EINVAL for a NULL image or g, H+1 < 4 or W+1 < 4, a dtype that is neither;
 * BT_EUNSUPPORTED for a side above BT_PATCH_MAX_SIDE.  bt_patch_generate: BT_EINVAL for NULL args, a NULL g, image, depth,
 * ux, uy or patches, H+1 < 4 or W+1 < 4, Hp != (H+1) div 4 or Wp != (W+1) div 4, G < 1, gm < 1, W_grid < 1 or H_grid < 1,
 * a bad dtype or rows_mode; BT_EUNSUPPORTED for 8*gm > BT_PATCH_MAX_CANDIDATES or a side above BT_PATCH_MAX_SIDE.
 * BT_EHIP if the launch fails.
 */
#ifndef BATRACK_PATCHES_H
#define BATRACK_PATCHES_H

#include <stddef.h>
#include <stdint.h>

#include "batrack_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BT_IMAGE_U8 0
#define BT_IMAGE_F32 1
#define BT_PATCH_ROWS_REFERENCE 0
#define BT_PATCH_ROWS_IMAGE 1
#define BT_PATCH_MAX_CANDIDATES 1024 /* C = 8*gm: a cell is ranked by one workgroup */
#define BT_PATCH_MAX_SIDE 32768

typedef struct {
    /* inputs */
    const float *g;                  /* [Hp, Wp] */
    int64_t Hp, Wp;                  /* must be (H+1) div 4, (W+1) div 4 */
    const void *image;               /* 3 channels of H x W, see the strides */
    int32_t dtype;                   /* BT_IMAGE_U8 | BT_IMAGE_F32 */
    int32_t rows_mode;               /* BT_PATCH_ROWS_REFERENCE | BT_PATCH_ROWS_IMAGE */
    int64_t H, W;
    int64_t stride_c, stride_y, stride_x;   /* in elements */
    const float *depth;              /* [H, W] */
    const float *ux, *uy;            /* [G*G, 8*gm] */
    int64_t G, gm;
    /* outputs */
    float *patches;                  /* [M, 3]  (px, py, disparity) */
    float *clr;                      /* [M, 3], may be NULL */
    uint8_t *colors;                 /* [M, 3], may be NULL */
    float *coords;                   /* [M, 2], may be NULL */
    int32_t *sel;                    /* [M], may be NULL */
} bt_patch_args;

int bt_image_gradient(const void *image, int32_t dtype, int64_t H, int64_t W, int64_t stride_c, int64_t stride_y,
                      int64_t stride_x, float *g, void *stream);

int bt_patch_generate(const bt_patch_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_PATCHES_H */
