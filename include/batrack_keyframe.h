/* batrack_keyframe.h — the last step of a frame of the reference's BATRACK.__call__, on the device (csrc/keyframe.hip):
 * `keyframe()` (main/batrack.py:1026-1073) with the two `motionmag` calls (:1011-1018) and the `remove_factors` rounds
 * (:206-212) it is built from, and `keyframe_simple()` (:1020-1024).  Three stages, separately callable, that talk to
 * each other through a status word in device memory, so nothing between them needs the host:
 *     (a) bt_keyframe_decide   the two mean flow magnitudes and the comparison with the threshold      2 launches (1 without a candidate)
 *     (b) bt_edges_prune       both removal rounds and the renumbering as ONE stable compaction         3 launches
 *     (c) bt_rows_shift        the per-frame buffers moved down by one row                              1 launch
 * No workgroup waits on another: every ordering comes from the kernel boundaries (no decoupled look-back, no tickets,
 * no spinning).  No float atomics: a call repeats bit for bit.
 *
 * Conventions of batrack_ba.h: DEVICE pointers only (the one exception is the descriptor array of bt_rows_shift, which
 * is read on the host and handed to the kernel by value), `stream` is a hipStream_t passed as void*, integer status
 * codes, every argument check returns before anything is enqueued, nothing allocates or synchronises.
 *
 * Workspace.  `workspace` is a caller-provided device buffer of bt_keyframe_workspace_bytes(E) bytes, 8-byte aligned,
 * E the largest edge count it is used with.  Its first sizeof(bt_keyframe_status) = 32 bytes ARE the status word; the
 * rest (the workgroups' partial sums, the tile counts and offsets) needs no initialisation.  Calls on one stream may
 * share it.  The caller reads the status by copying the first 32 bytes to the host, once, after the last stage.
 *
 * (a) bt_keyframe_decide.  With k the candidate frame, an edge e is selected as `prev` if jj[e] == k && ii[e] == k-1 and
 * as `next` if jj[e] == k && ii[e] == k+1 (`motionmag(k-1, k)`, `motionmag(k+1, k)`).  A selected edge computes the
 * reference's flow_mag (projective_ops.py:112-122) at the centre pixel (p/2, p/2) of its patch:
 *     c0 = reproject(ii -> ii),  c1 = reproject(ii -> jj),  c2 = reproject(ii -> jj, translation only)
 *     f  = f32(beta) * |c1 - c0| + f32(1 - beta) * |c2 - c0|              |.| = sqrtf(dx*dx + dy*dy)
 * in float32, each reprojection by the same device function as bt_reproject (batrack_projective.h; G_i * G_i^-1 is
 * computed as such).  A selected edge with ii, jj outside [0, n_poses) or kk outside [0, n_patches) contributes NaN, as
 * in bt_reproject.  The f are added in double: a thread adds the edges it visits in index order, a workgroup adds its
 * threads' sums in a fixed tree, and one thread of a second kernel adds the workgroups' partials in index order; the
 * grid is a function of E alone.  Then
 *     mag_prev = (float)(sum_prev / cnt_prev)      (cnt == 0: NaN, as torch.mean of an empty tensor), mag_next alike
 *     removed  = ((double)mag_prev + (double)mag_next) / 2 < thresh            IEEE: false when either mean is NaN
 * so a pair without edges never removes a frame (k = 0, k = n-1).  k = -1 means "no candidate" (keyframe_simple): the
 * edge list is not read, removed = 0, both magnitudes NaN, both counts 0.
 * Writes: removed, mag_prev, mag_next, cnt_prev, cnt_next of the status.  E_out is not written.  Inputs are not written.
 * Return: BT_EINVAL for a NULL workspace, E < 0, k < -1, and — when k >= 0 and E > 0 — a NULL input, n_poses < 0,
 * n_patches < 0, patch_elems not a square in [1, 4096]; BT_EUNSUPPORTED for E > 2^31 - 1; BT_EHIP if a launch fails.
 *
 * (b) bt_edges_prune.  With r = status.removed (read on the device), per edge e in input order:
 *     if r and (ii == k or jj == k):                      drop                                   batrack.py:1045-1046
 *     if r: kk' = kk - M*(ii > k); ii' = ii - (ii > k); jj' = jj - (jj > k); n' = n - 1          :1048-1050
 *     else: kk' = kk; ii' = ii; jj' = jj; n' = n
 *     if floor(kk' / M) < n' - removal_window:            drop      :1072 (ix[kk] is kk div M: index_[f] = f, never shifted)
 *     else write (ii', jj', kk', targets_3d[e], weights[e], weights_pose[e]) at row rank(e), the number of kept edges before e
 * status.E_out = the number kept.  Rows >= E_out of the outputs are NOT written; the inputs are NOT modified; of the
 * status only E_out is written.  k < 0 never matches an edge's frame; with r == 0 only the removal window applies.
 * Three passes: kept count per tile of bt_edges_prune_tile() edges (wave ballot + popcount); exclusive scan of the tile
 * counts by one workgroup, bt_edges_prune_scan_span() counts per pass with a carry; scatter (predicate recomputed, rank
 * = tile offset + the preceding waves' counts + ballot & lanes-below popcount).
 *   ii, jj, kk [E] int64;  targets_3d [E,3], weights [E,2], weights_pose [E,2] float32;  the six outputs likewise, each of
 *   capacity E.  The work is out of place: an output that overlaps an input, another output or the workspace is
 *   BT_EINVAL (the inputs are only read).
 * Return: BT_EINVAL for a NULL workspace, E < 0, M < 1, and — when E > 0 — a NULL buffer, a buffer that is not 8-byte
 * aligned (targets_3d: 4-byte) or an output that overlaps an input, another output or the workspace; BT_EUNSUPPORTED for E > 2^31 - 1.  E = 0 is BT_OK with E_out = 0 (one launch;
 * the buffers are not looked at).  BT_EHIP if a launch fails.
 *
 * (c) bt_rows_shift.  bufs[b] = (ptr, row_bytes), b < nbuf <= BT_KEYFRAME_MAX_BUFFERS: a device buffer of at least n rows
 * of row_bytes bytes.  If status.removed (read on the device): row[i] = row[i+1] for i = k .. n-2 in every buffer; row
 * n-1 keeps its content, as the loop at batrack.py:1052-1063 leaves it; rows < k and bytes outside the n rows are not
 * touched.  Each thread owns a column unit — 4 bytes where row_bytes % 4 == 0 and ptr is 4-byte aligned, one byte
 * otherwise — and walks the rows in order, so no thread reads what another writes.  removed == 0 touches nothing.
 * The status is not written.
 * Return: BT_EINVAL for a NULL workspace, nbuf < 0 or > BT_KEYFRAME_MAX_BUFFERS, and — when nbuf > 0 — NULL bufs, a NULL
 * ptr, row_bytes < 1, k < 0, n < 0.  nbuf == 0 or k >= n - 1 is BT_OK and enqueues nothing.  BT_EHIP if the launch fails.
 */
#ifndef BATRACK_KEYFRAME_H
#define BATRACK_KEYFRAME_H

#include <stddef.h>
#include <stdint.h>

#include "batrack_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BT_KEYFRAME_MAX_BUFFERS 16

typedef struct {
    int64_t removed;                 /* (a): 1 if the candidate frame is to be removed, else 0 */
    int64_t E_out;                   /* (b): edges kept */
    float mag_prev, mag_next;        /* (a): mean flow magnitude over the edges (k-1 -> k), (k+1 -> k) */
    int32_t cnt_prev, cnt_next;      /* (a): how many edges each mean is over */
} bt_keyframe_status;                /* 32 bytes, the head of the workspace */

typedef struct {
    void *ptr;                       /* device buffer, rows of row_bytes bytes */
    int64_t row_bytes;
} bt_row_buffer;

size_t bt_keyframe_workspace_bytes(int64_t E);
int64_t bt_edges_prune_tile(void);        /* edges per workgroup of the count and scatter passes */
int64_t bt_edges_prune_scan_span(void);   /* tile counts the scan takes per pass */

int bt_keyframe_decide(int64_t k, const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E, const float *poses,
                       int64_t n_poses, const float *patches, int64_t n_patches, int64_t patch_elems, const float *intrinsics,
                       double beta, double thresh, void *workspace, void *stream);

int bt_edges_prune(int64_t k, int64_t n, int64_t M, int64_t removal_window, const int64_t *ii, const int64_t *jj,
                   const int64_t *kk, const float *targets_3d, const float *weights, const float *weights_pose, int64_t E,
                   int64_t *ii_out, int64_t *jj_out, int64_t *kk_out, float *targets_3d_out, float *weights_out,
                   float *weights_pose_out, void *workspace, void *stream);

int bt_rows_shift(const bt_row_buffer *bufs, int32_t nbuf, int64_t k, int64_t n, const void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_KEYFRAME_H */
