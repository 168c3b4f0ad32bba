/* batrack_projective.h — C ABI of the fused reprojection and of the world-frame point cloud / 3-D track trajectories
 * (SURVEY.md §8 row f-3).
 *
 * Replaces, for the non-Jacobian call of the reference's
 *     pops.transform(poses, patches, intrinsics, ii, jj, kk, depth=, valid=, tonly=)
 *                /root/reference/main/backend/projective_ops.py:54-75,102-105
 * the chain iproj (:19-29) -> Gij = G_j * G_i^-1 (lietorch inv, mul) -> act4 -> proj (:32-52), which the caller
 * runs once per frame over the whole edge list for its map filtering (batrack.py:327-338), for `flow_mag`
 * (:1017, projective_ops.py:112-122) and for the point-cloud export.  One thread per (edge, patch pixel); the
 * group arithmetic follows the same sequence of float32 operations as the element-wise kernels of batrack_se3.h.
 *
 * All pointers are DEVICE pointers, contiguous:
 *   poses       [n_poses, 7]   tx ty tz qx qy qz qw (re-normalised on load)
 *   patches     [n_patches, 3, p, p]   planes x, y, inverse depth; patch_elems = p*p
 *   intrinsics  [n_poses, 4]   fx fy cx cy
 *   ii, jj, kk  [E] int64      source frame, target frame, patch of every edge
 *   coords      [E, p, p, 2]   (u, v), or [E, p, p, 3] = (u, v, projected inverse depth) with BT_REPROJECT_DEPTH
 *   valid       [E, p, p]      1.0 where Z > 0.2 else 0.0; may be NULL
 * An edge with an index out of range yields NaN coordinates and valid = 0 (the reference's gather would raise).
 * Z is clamped at 1e-2 before the division (projective_ops.py:43).
 * Return: BT_OK (0) / BT_EINVAL (-1) / BT_EHIP (-3), as in batrack_ba.h.
 */
#ifndef BATRACK_PROJECTIVE_H
#define BATRACK_PROJECTIVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BT_REPROJECT_DEPTH 1   /* also emit the projected inverse depth (proj(..., depth=True))        */
#define BT_REPROJECT_TONLY 2   /* translation-only relative motion (transform(..., tonly=True), :61-64) */

int bt_reproject(const float *poses, int64_t n_poses, const float *patches, int64_t n_patches, int64_t patch_elems,
                 const float *intrinsics, const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E,
                 int32_t mode, float *coords, float *valid, void *stream);

/* bt_world_tracks — the last statements of the reference's per-frame update() in one launch (csrc/world_tracks.hip):
 * the world-frame point cloud (`points_`, batrack.py:891-893), the 3-D trajectories of the tracks over their windows
 * (`trajs_3d_world`, update_point_cloud :821-845) and the overwrite of the live tracks' window buffer by the
 * re-projection of their world point (:847-854), which is the depth prior of the next BA calls (:866) and
 * `trajs_2d_disp` of results.pkl.
 *
 * All pointers are DEVICE pointers, contiguous, float32 unless noted:
 *   poses          [N, 7]            world -> camera, tx ty tz qx qy qz qw (re-normalised on load); N = n_poses
 *   intrinsics     [N, 4]            fx fy cx cy
 *   patches        [n_patches, 3, p, p]   planes x, y, inverse depth; patch_elems = p*p (a square, <= 4096); the centre
 *                                    pixel (p/2, p/2) is the track; n_patches = N*M, the whole buffer
 *   ix             [>= m] int64      source frame of a track
 *   patches_local  [n_patches, S_local, 3]   IN/OUT: (u, v, inverse depth) of a track in the S_local frames around its own
 *   local_weights  [n_patches, S_local]      the tracks' window weights
 *   points         [>= m, 3]         out, may be NULL (not written)
 *   world          [n_patches, S_local, 3]   out, may be NULL (not written)
 * With mid = (S_local + 1)/2 - 1, for every track k < m and i = ix[k]:
 *     live_k = sum_s local_weights[k, s] > 0        (four interleaved partial sums, then added pairwise)
 *     X0     = ((x - cx_i)/fx_i, (y - cy_i)/fy_i, 1, d)              (x, y, d) = centre of patches[k]
 *     Pw     = G_i^-1 * X0         homogeneous: (R_i^T (X0_123 - t_i d), d)
 *     points[k] = Pw_123 / d
 *     for s in 0 .. S_local-1:   j = clamp(i + s - mid, 0, N - 1)         (N, the buffer, not the frames seen)
 *       live_k:      world[k, s] = points[k]
 *                    Xc = G_j * Pw ;  r = 1 / max(Xc_3, 1e-2)
 *                    patches_local[k, s] = (fx_j (r Xc_1) + cx_j, fy_j (r Xc_2) + cy_j, r d)
 *       not live_k:  (u, v, e) = patches_local[k, s]
 *                    Wd = G_j^-1 * ((u - cx_j)/fx_j, (v - cy_j)/fy_j, 1, e)
 *                    world[k, s] = Wd_123 / e ;  patches_local[k, s] unchanged
 * Tracks k >= m are not touched.  Divisions follow IEEE: a slot that was never filled (e = 0) gives a non-finite world
 * point, as in the reference.  An ix[k] outside [0, N) gives NaN for that track: its point, its world row and, if it is
 * live, its patches_local row.  float32 arithmetic in the operation order of the element-wise kernels of batrack_se3.h
 * (inv, then act4).  No atomics: a call repeats bit for bit.  Nothing allocates or synchronises.
 * Return: BT_EINVAL for a NULL input, N < 1, S_local < 1, patch_elems < 1 or not a square <= 4096, m < 0 or m > n_patches;
 * BT_EUNSUPPORTED for S_local > 2^20 or N > 2^30 — all before anything is enqueued; m = 0 is BT_OK; BT_EHIP if the launch
 * fails. */
int bt_world_tracks(const float *poses, int64_t n_poses, const float *intrinsics, const float *patches, int64_t n_patches,
                    int64_t patch_elems, const int64_t *ix, float *patches_local, const float *local_weights,
                    int64_t S_local, int64_t m, float *points, float *world, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_PROJECTIVE_H */
