// world_tracks.hip — the last statements of the caller's per-frame update() fused for gfx950: the world point of every
// track, its 3-D trajectory over the S_local frames around its own, and the re-projection of live tracks' world points
// into their window (specification: include/batrack_projective.h, bt_world_tracks).
// Formulas: /root/reference/main/batrack.py:821-854,891-893, backend/projective_ops.py:19-52,107-109, lietorch se3.h:36-56.
//
// One workgroup takes WT_TRACKS consecutive tracks.  Phase 1, four lanes a track: the window's weight sum (`live`) and
// Pw = G_i^-1 X0, once per track, into LDS; `points` is written here.  Phase 2, lanes over the flattened (track, slot)
// index of the block, so that the 12-byte records of `patches_local` and `world` are contiguous across a wave (dwordx3
// loads and stores, 768 B a wave).  The pose and intrinsics rows a block needs (the <= S_local frames around its
// tracks' own, 44 B each) are read through the cache.  A live slot does not read its `patches_local` record; a slot that
// is not live does not write it.  No atomics: a call repeats bit for bit.
// float32 in the operation order of se3_kernels.hip (inv = conj + rotate, act4 = rotate + t * d), the quaternion
// re-normalised wherever the separate kernels would load it, with the same fused multiply-adds (see below).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_projective.h"

namespace bt {

constexpr int WT_TRACKS = 64;      // tracks of one workgroup
constexpr int WT_THREADS = 256;

struct WF3 { float x, y, z; };     // one 12-byte record, 4-byte aligned
struct WQ { float x, y, z, w; };
struct WPose { float t[3]; WQ q; };

// The group arithmetic is written out with the fused multiply-adds the compiler forms in k_se3_inv / k_se3_act
// (se3_kernels.hip, -ffp-contract=fast), and contraction is off for the rest of this file: the pinhole arithmetic
// around it rounds every operation, as the composed tensor operations do.  The kernel then agrees with the separate
// calls bit for bit wherever its inputs do, instead of by whichever products the compiler happens to fuse here.
#pragma clang fp contract(off)

__device__ __forceinline__ WQ wt_unit(WQ q) {                                                  // so3.h:35-37
    const float n = 1.0f / sqrtf(fmaf(q.w, q.w, fmaf(q.z, q.z, fmaf(q.x, q.x, q.y * q.y))));
    return {q.x*n, q.y*n, q.z*n, q.w*n};
}
__device__ __forceinline__ WPose wt_load_pose(const float *__restrict__ d) {
    return {{d[0], d[1], d[2]}, wt_unit({d[3], d[4], d[5], d[6]})};
}
__device__ __forceinline__ void wt_rot(WQ q, const float *p, float *o) {                       // so3.h:55-60
    float ux = fmaf(q.y, p[2], -(q.z * p[1])), uy = fmaf(q.z, p[0], -(q.x * p[2])), uz = fmaf(q.x, p[1], -(q.y * p[0]));
    ux += ux; uy += uy; uz += uz;
    o[0] = fmaf(q.w, ux, p[0]) + fmaf(q.y, uz, -(q.z * uy));
    o[1] = fmaf(q.w, uy, p[1]) + fmaf(q.z, ux, -(q.x * uz));
    o[2] = fmaf(q.w, uz, p[2]) + fmaf(q.x, uy, -(q.y * ux));
}
// G^-1 * (X, d) = (R^T X - (R^T t) d, d): inv (se3.h:36-38) then act4 (:53-56)
__device__ __forceinline__ void wt_inv_act4(const WPose &g, const float *X, float d, float *o) {
    const WQ qi = wt_unit({-g.q.x, -g.q.y, -g.q.z, g.q.w});
    float tt[3], r[3];
    wt_rot(qi, g.t, tt);                           // the inverse's translation, from the quaternion inv normalised
    wt_rot(wt_unit(qi), X, r);                     // the inverse is a pose of its own: re-normalised when act4 loads it
    o[0] = fmaf(d, -tt[0], r[0]); o[1] = fmaf(d, -tt[1], r[1]); o[2] = fmaf(d, -tt[2], r[2]);
}

__global__ __launch_bounds__(WT_THREADS) void k_world_tracks(const float *__restrict__ poses, int64_t N,
                                                              const float *__restrict__ intr,
                                                              const float *__restrict__ patches, int pe, int centre,
                                                              const int64_t *__restrict__ ix, float *plocal,
                                                              const float *__restrict__ lw, int64_t m, int S, int mid,
                                                              float *__restrict__ points, float *__restrict__ world) {
    __shared__ float s_pw[4][WT_TRACKS];           // Pw = (x, y, z, d) of the block's tracks
    __shared__ float s_pt[3][WT_TRACKS];           // the world point Pw_xyz / d
    __shared__ int s_i[WT_TRACKS];                 // source frame, -1: out of range
    __shared__ int s_live[WT_TRACKS];
    const int tid = threadIdx.x;
    const int64_t nblk = (m + WT_TRACKS - 1) / WT_TRACKS;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        const int64_t k0 = b * WT_TRACKS;
        const int nt = (int)(m - k0 < WT_TRACKS ? m - k0 : WT_TRACKS);
        // ---- phase 1: per track, lanes 4t .. 4t+3 share the weight sum
        {
            const int t = tid >> 2, part = tid & 3;
            const bool on = t < nt;
            float acc = 0.0f;
            if (on) {
                const float *w = lw + (k0 + t) * (int64_t)S;
                for (int s = part; s < S; s += 4) acc += w[s];
            }
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            if (on && part == 0) {
                const int64_t k = k0 + t, i = ix[k];
                const bool ok = i >= 0 && i < N;
                float P[3] = {NAN, NAN, NAN}, d = NAN;
                if (ok) {
                    const float *pat = patches + (size_t)k * 3 * pe + centre, *K = intr + 4 * i;
                    d = pat[2 * pe];
                    const float X0[3] = {(pat[0] - K[2]) / K[0], (pat[pe] - K[3]) / K[1], 1.0f};  // projective_ops.py:19-29
                    wt_inv_act4(wt_load_pose(poses + 7 * i), X0, d, P);
                }
                s_pw[0][t] = P[0]; s_pw[1][t] = P[1]; s_pw[2][t] = P[2]; s_pw[3][t] = d;
                s_i[t] = ok ? (int)i : -1;
                s_live[t] = acc > 0.0f;
                const WF3 pt = {P[0] / d, P[1] / d, P[2] / d};
                s_pt[0][t] = pt.x; s_pt[1][t] = pt.y; s_pt[2][t] = pt.z;
                if (points) *reinterpret_cast<WF3 *>(points + 3 * k) = pt;
            }
        }
        __syncthreads();
        // ---- phase 2: per (track, slot)
        const unsigned tot = (unsigned)nt * (unsigned)S;
        for (unsigned f = tid; f < tot; f += WT_THREADS) {
            const unsigned t = f / (unsigned)S;
            const int s = (int)(f - t * (unsigned)S);
            const int64_t slot = k0 * (int64_t)S + f;
            const int i = s_i[t];
            const bool live = s_live[t];
            const float d = s_pw[3][t];
            const float Pw[3] = {s_pw[0][t], s_pw[1][t], s_pw[2][t]};
            WF3 *pl = reinterpret_cast<WF3 *>(plocal + 3 * slot);
            WF3 wp = {NAN, NAN, NAN};
            if (i < 0) {
                if (live) *pl = wp;
            } else {
                int64_t j = (int64_t)i + s - mid;
                j = j < 0 ? 0 : (j > N - 1 ? N - 1 : j);                                     // batrack.py:833-834
                const WPose g = wt_load_pose(poses + 7 * j);
                const float *K = intr + 4 * j;
                if (live) {
                    wp = {s_pt[0][t], s_pt[1][t], s_pt[2][t]};
                    float r[3];
                    wt_rot(g.q, Pw, r);                                                      // act4, se3.h:53-56
                    const float X = fmaf(d, g.t[0], r[0]), Y = fmaf(d, g.t[1], r[1]), Z = fmaf(d, g.t[2], r[2]);
                    const float iz = 1.0f / fmaxf(Z, 1e-2f);                                 // projective_ops.py:43
                    *pl = WF3{K[0] * (iz * X) + K[2], K[1] * (iz * Y) + K[3], iz * d};
                } else {
                    const WF3 q = *pl;
                    const float Xd[3] = {(q.x - K[2]) / K[0], (q.y - K[3]) / K[1], 1.0f};
                    float W[3];
                    wt_inv_act4(g, Xd, q.z, W);
                    wp = {W[0] / q.z, W[1] / q.z, W[2] / q.z};
                }
            }
            if (world) *reinterpret_cast<WF3 *>(world + 3 * slot) = wp;
        }
        __syncthreads();
    }
}

}  // namespace bt

extern "C" int bt_world_tracks(const float *poses, int64_t n_poses, const float *intrinsics, const float *patches,
                               int64_t n_patches, int64_t patch_elems, const int64_t *ix, float *patches_local,
                               const float *local_weights, int64_t S_local, int64_t m, float *points, float *world,
                               void *stream) {
    if (n_poses < 1 || n_patches < 0 || patch_elems < 1 || S_local < 1 || m < 0 || m > n_patches) return BT_EINVAL;
    if (!poses || !intrinsics || !patches || !ix || !patches_local || !local_weights) return BT_EINVAL;
    int64_t p = (int64_t)std::sqrt((double)patch_elems);
    while (p * p > patch_elems) --p;
    while ((p + 1) * (p + 1) <= patch_elems) ++p;
    if (p * p != patch_elems || patch_elems > 4096) return BT_EINVAL;             // a p x p patch, as bt_reproject bounds it
    if (S_local > (1 << 20) || n_poses > (1 << 30)) return BT_EUNSUPPORTED;      // 32-bit slot index inside a workgroup
    if (m == 0) return BT_OK;
    int64_t nb = (m + bt::WT_TRACKS - 1) / bt::WT_TRACKS;
    if (nb > 2048) nb = 2048;                      // 256 CUs x 8 resident workgroups; the kernel strides over the rest
    hipLaunchKernelGGL(bt::k_world_tracks, dim3((unsigned)nb), dim3(bt::WT_THREADS), 0, static_cast<hipStream_t>(stream),
                       poses, n_poses, intrinsics, patches, (int)patch_elems, (int)((p / 2) * (p + 1)), ix, patches_local,
                       local_weights, m, (int)S_local, (int)((S_local + 1) / 2 - 1), points, world);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
