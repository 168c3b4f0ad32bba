/* batrack_observe.h — the step between the tracker's forward pass and the bundle adjustment, on the device
 * (csrc/observe.hip): the tail of `_compute_sparse_tracks`, `get_window_trajs`, `predict_target` and `update_local` of
 * the reference's BATRACK (main/batrack.py:575-587, 667-757, 760-818, 632-663).  From the network's window output it
 * makes the new edges' targets and weights, the motion-decoupled pose weights, the `patches_valid_` rows of the window's
 * keyframes, the queries' mono disparity, and scatters five values per edge into the tracks' window buffers.
 *
 * Conventions of batrack_ba.h: DEVICE pointers only, `stream` is a hipStream_t passed as void*, integer status codes,
 * every argument check returns before anything is enqueued, nothing allocates or synchronises.  No float atomics: a call
 * repeats bit for bit.  A call is at most three launches of fixed shape (query sampling, one workgroup for the
 * threshold, the window pass); the threshold never leaves device memory: it lives in a caller-provided workspace of
 * bt_observe_workspace_bytes() bytes, which needs no initialisation and may be reused by the next call on the stream.
 *
 * Notation.  S: the padded window length (the tracker's S_slam).  S' = Sp <= S: the frames really in the window.
 * Nq = Q*M queries: the M tracks of Q = ceil(S'/kf_stride) keyframes, every kf_stride-th frame from lo = n - S'.
 * E = Nq*S' new edges, track-major: e = q*S' + s (the reference's 'b s n c -> b (n s) c').
 * row(q) = (lo + kf_stride*(q / M), q mod M) is the query's row of patches_valid.
 *
 * All arithmetic is float32 in the reference's operation order, every operation rounded (no contraction); the division
 * is the correctly rounded one.
 *   1. tracker tail, when interp_w > 0: with t_q = (int)queries[q,0], sx = f32(interp_w/W), rx = f32(W/interp_w) (the
 *      quotients taken in double) and sy, ry likewise from interp_h and H:
 *        x[s,q] = (s == t_q ? queries[q,1]*sx : traj[s,q,0]) * rx,   y likewise,   vis[t_q,q] = 1.
 *      With interp_w == 0 traj and vis are taken as they are.  The inputs are not written.
 *   2. query depth, when dmaps != NULL: d = bilinear sample of dmaps[t_q] at the unscaled (qx, qy) = queries[q,1:3]:
 *      x0 = floor(qx), x1 = x0 + 1 (y alike), the four indices clamped to the map, the weights from the unclamped corners,
 *        d = (((x1-qx)(y1-qy)) I00 + ((qx-x0)(y1-qy)) I01) + ((x1-qx)(qy-y0)) I10) + ((qx-x0)(qy-y0)) I11
 *      query_disp[q] = 1 / (d < 1e-2 ? 1e-2 : d)    (a NaN d stays NaN).  A t_q outside [0, S') gives NaN.
 *   3. vis_label = vis > vis_threshold (all true with has_vis_threshold == 0);
 *      inside = x >= pad && x < f32(wd - pad) && y >= pad && y < f32(ht - pad);   vis_raw = vis_label && inside.
 *   4. static = 1 - dyn;  th = the quantile f32(1 - static_quantile) of ALL S*Nq values of static (the padded frames
 *      included), torch.quantile's linear interpolation: rank = qf * f32(S*Nq - 1), a = the floor(rank)-th and b = the
 *      ceil(rank)-th smallest, w = rank - floor(rank), w < 0.5 ? fma(w, b - a, a) : fma(w - 1, b - a, b);
 *      then th = static_threshold < th ? static_threshold : th.   static_label = static >= th.
 *      A NaN anywhere in dyn makes th NaN and no entry static (Python's min(nan, x) is nan).
 *   5. when is_initialized: patches_valid[row(q)] = patches_valid[row(q)] != 0 || (sum_{s<S'} vis_label[s,q]) > 3.
 *   6. targets_3d[e] = (x, y, 1 / (depth < 1e-2 ? 1e-2 : depth))   (a NaN depth stays NaN);  w = vis_raw ? 1 : 0;
 *      when n >= min_track_len: pv_q = (sum_{s<S'} vis_raw[s,q]) >= min_track_len; patches_valid[row(q)] = pv_q
 *      (overwriting 5.) and w = 0 for the tracks with !pv_q.   weights[e] = (w, w).
 *   7. weights_pose[e] = static_label ? (w, w) : (0, 0).
 *   8. slot = jj[e] - ii[e] + (S_local + 1)/2 - 1; for 0 <= slot < S_local and 0 <= kk[e] < N*M:
 *        patches_local[kk,slot] = target, local_monodisp[kk,slot] = target disparity, local_vis[kk,slot] = vis_raw,
 *        local_static[kk,slot] = static_label, local_weights[kk,slot] = w   (each of the last four only if not NULL).
 *      Other edges write no buffer.  A (kk, slot) pair that occurs twice in one call is the caller's error.
 */
#ifndef BATRACK_OBSERVE_H
#define BATRACK_OBSERVE_H

#include <stddef.h>
#include <stdint.h>

#include "batrack_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BT_OBSERVE_MAX_S 64          /* the window pass keeps a (track, frame) tile in LDS */

typedef struct {
    /* sizes */
    int64_t S, Sp, Nq, E;            /* E must equal Nq*Sp */
    int64_t n, M, N, kf_stride, S_local;
    int64_t H, W;                    /* the images' size: the tail's rescale and the depth maps */
    int64_t interp_w, interp_h;      /* 512, 384 in the reference; both 0 = no tail */
    int64_t padding, min_track_len;
    int32_t has_vis_threshold, is_initialized;
    double wd, ht;                   /* the image bounds of `inside` (the reference's self.wd, self.ht) */
    double vis_threshold, static_quantile, static_threshold;
    /* inputs, float32 contiguous unless noted */
    const float *traj;               /* [S, Nq, 2] */
    const float *depth, *vis, *dyn;  /* [S, Nq] */
    const float *queries;            /* [Nq, 3]  (t, x, y), full-image pixels */
    const float *dmaps;              /* [Sp, H, W], may be NULL: no query sampling, query_disp not written */
    const int64_t *ii, *jj, *kk;     /* [E] */
    /* in/out */
    float *patches_valid;            /* [N, M] */
    float *patches_local;            /* [N*M, S_local, 3] */
    float *local_monodisp, *local_vis, *local_static, *local_weights;   /* [N*M, S_local], each may be NULL */
    /* outputs */
    float *targets_3d;               /* [E, 3] */
    float *weights, *weights_pose;   /* [E, 2] */
    float *query_disp;               /* [Nq], may be NULL when dmaps is NULL */
} bt_observe_args;

size_t bt_observe_workspace_bytes(void);

/* Return: BT_EINVAL for a NULL args / workspace / required pointer (query_disp is required with dmaps), S < 1, Sp < 0 or
 * > S, Nq < 0, M < 1, Nq not Q*M with Q = ceil(Sp/kf_stride), E != Nq*Sp, kf_stride < 1, N < 1, n < Sp or n > N,
 * S_local < 1, H < 1 or W < 1, interp_w / interp_h negative or only one of them 0, padding < 0, static_quantile outside
 * [0, 1] or NaN; BT_EUNSUPPORTED for S > BT_OBSERVE_MAX_S, S*Nq >= 2^24 (the float32 rank), N*M*S_local >= 2^31 or
 * H*W >= 2^31.  E = 0 is BT_OK and touches nothing (the pointers are
 * not looked at then).  BT_EHIP if a launch fails. */
int bt_observe_window(const bt_observe_args *args, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_OBSERVE_H */
