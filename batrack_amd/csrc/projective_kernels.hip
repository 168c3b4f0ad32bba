// projective_kernels.hip — fused reprojection of patches along the edge list for gfx950:
// iproj -> G_j * G_i^-1 -> act4 -> proj in one pass, one thread per (edge, patch pixel).
// Formulas: /root/reference/main/backend/projective_ops.py:19-75, lietorch/include/se3.h:36-56, so3.h:31-60.
// HBM-bound gather: 24 B of indices + 12 B of patch per edge read, 8-16 B written; the pose and
// intrinsics tables (<= 1024 rows) stay in cache.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_projective.h"
#include "projective_edge.hpp"

namespace bt {

template <bool DEPTH, bool TONLY>
__global__ __launch_bounds__(256) void k_reproject(const float *__restrict__ poses, int64_t n_poses,
                                                   const float *__restrict__ patches, int64_t n_patches, int pe,
                                                   const float *__restrict__ intr, const int64_t *__restrict__ ii,
                                                   const int64_t *__restrict__ jj, const int64_t *__restrict__ kk,
                                                   int64_t total, float *__restrict__ coords, float *__restrict__ valid) {
    constexpr int NO = DEPTH ? 3 : 2;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = pe == 1 ? t : t / pe;
        const int pix = pe == 1 ? 0 : (int)(t - e * pe);
        const int64_t i = ii[e], j = jj[e], k = kk[e];
        float *out = coords + t * NO;
        if (i < 0 || j < 0 || k < 0 || i >= n_poses || j >= n_poses || k >= n_patches) {
            out[0] = out[1] = NAN;
            if (DEPTH) out[2] = NAN;
            if (valid) valid[t] = 0.0f;
            continue;
        }
        const float *pat = patches + (size_t)k * 3 * pe + pix;
        const float Z = reproject_pixel<DEPTH, TONLY>(poses + 7 * i, poses + 7 * j, intr + 4 * i, intr + 4 * j, pat, pe, out);   // projective_edge.hpp
        if (valid) valid[t] = Z > 0.2f ? 1.0f : 0.0f;                                       // projective_ops.py:103
    }
}

}  // namespace bt

extern "C" int bt_reproject(const float *poses, int64_t n_poses, const float *patches, int64_t n_patches, int64_t patch_elems,
                            const float *intrinsics, const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E,
                            int32_t mode, float *coords, float *valid, void *stream) {
    if (E < 0 || n_poses < 0 || n_patches < 0 || patch_elems <= 0 || patch_elems > 4096 || (mode & ~3)) return BT_EINVAL;
    if (E == 0) return BT_OK;
    if (!poses || !patches || !intrinsics || !ii || !jj || !kk || !coords) return BT_EINVAL;
    const int64_t total = E * patch_elems;
    int64_t nb = (total + 255) / 256;
    if (nb > 16384) nb = 16384;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)nb), blk(256);
    const int pe = (int)patch_elems;
    switch (mode) {
    case 0: hipLaunchKernelGGL((bt::k_reproject<false, false>), grid, blk, 0, st, poses, n_poses, patches, n_patches, pe, intrinsics, ii, jj, kk, total, coords, valid); break;
    case 1: hipLaunchKernelGGL((bt::k_reproject<true, false>), grid, blk, 0, st, poses, n_poses, patches, n_patches, pe, intrinsics, ii, jj, kk, total, coords, valid); break;
    case 2: hipLaunchKernelGGL((bt::k_reproject<false, true>), grid, blk, 0, st, poses, n_poses, patches, n_patches, pe, intrinsics, ii, jj, kk, total, coords, valid); break;
    default: hipLaunchKernelGGL((bt::k_reproject<true, true>), grid, blk, 0, st, poses, n_poses, patches, n_patches, pe, intrinsics, ii, jj, kk, total, coords, valid); break;
    }
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
