// video_prep.hip — k_frame_prep, the tracker's input preparation (include/batrack_video.h holds the specification): the
// bilinear resize of F frames' colour and depth to the tracker's size with the exact source coordinate, the colour mapping
// to [-1, 1], and each frame's masked depth range, in one launch.
//
//   lane     BT_VIDEO_VEC = 4 neighbouring output columns of one output row: the row's taps and weights and the four columns'
//            are computed once and serve all four planes; each plane's four values leave in one 16-byte store (element by
//            element when the row length or the pointer does not allow it: the same values).
//   block    256 lanes on consecutive groups of four columns, row after row (BT_VIDEO_TILE = 1024 pixels a trip), so that a
//            wave's stores are one contiguous 1 KB run per plane.  blockIdx.y is the frame, blockIdx.x the share of it.
//   range    each lane folds its depth values into a (min, max) as it writes them; the frame's blocks meet in the reduction
//            of minmax_reduce.hpp, on the frame's own ticket and pairs.
// Memory-bound: at 480 x 854 -> 384 x 512 a frame reads 1.6 MB (uint8) or 6.6 MB (float32) and writes 3.1 MB.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_video.h"
#include "conv_tile.hpp"
#include "minmax_reduce.hpp"

// Every product and sum below is rounded on its own: written with plain operators under `fp contract(off)`, as sample_taps.hpp
// does.  (The __fmul_rn / __fadd_rn intrinsics are plain operators in a header the pragma does not reach, and fuse.)
#pragma clang fp contract(off)

namespace bt {

constexpr int FP_THREADS = WD_THREADS, FP_VEC = BT_VIDEO_VEC;
static_assert(FP_THREADS * FP_VEC == BT_VIDEO_TILE && FP_VEC == 4, "a lane stores one float4 per plane");

struct SrcTap { int i0, i1; float l0, l1; };

// the source taps of output index o of n_out over n_in, the coordinate exact (batrack_video.h).  SMALL: (2 n_out + 1) n_in
// fits 31 bits and 2 n_out is below 2^24, so 32-bit integers and a float32 quotient of exact operands do.  Otherwise 64-bit
// integers, and the float64 quotient rounded to float32 (two roundings) only where 2 n_out does not fit a float32 exactly.
template <bool SMALL>
__device__ __forceinline__ SrcTap src_tap(int o, int n_in, int n_out) {
    SrcTap t;
    if (SMALL) {
        const int s = (2 * o + 1) * n_in - n_out;
        const unsigned num = s > 0 ? (unsigned)s : 0u, den = 2u * (unsigned)n_out;
        t.i0 = (int)(num / den);
        t.l1 = __fdiv_rn((float)(num % den), (float)den);
    } else {
        const long long s = (2LL * o + 1) * n_in - n_out;
        const unsigned long long num = s > 0 ? (unsigned long long)s : 0ull, den = 2ull * (unsigned long long)n_out;
        t.i0 = (int)(num / den);
        const unsigned long long rem = num % den;               // both exact in float32 below 2^24: one rounding there too
        t.l1 = den < (1ull << 24) ? __fdiv_rn((float)rem, (float)den) : (float)__ddiv_rn((double)rem, (double)den);
    }
    t.l0 = 1.0f - t.l1;
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    return t;
}

__device__ __forceinline__ float blend(float a, float b, float c, float d, const SrcTap &ty, const SrcTap &tx) {
#pragma clang fp contract(off)
    const float top = tx.l0 * a + tx.l1 * b;
    const float bot = tx.l0 * c + tx.l1 * d;
    return ty.l0 * top + ty.l1 * bot;
}

// 2 (v / 255) - 1, md_tracker.py:435: the division correctly rounded, then two rounded operations
__device__ __forceinline__ float unit_colour(float v) {
#pragma clang fp contract(off)
    const float q = __fdiv_rn(v, 255.0f);
    return 2.0f * q - 1.0f;
}

struct FramePrepArgs {
    const void *image; const float *depth;
    long long si_f, si_c, si_y, si_x, sd_f, sd_y, sd_x;
    int F, H, W, oh, ow, groups_x;               // groups_x = ceil(ow / 4)
    long long groups;                            // oh * groups_x
    int is_u8, normalise, use_log, vec;
    float *part; unsigned *ticket; float *rgbd, *drange;
};

template <bool SMALL>
__global__ __launch_bounds__(FP_THREADS) void k_frame_prep(const FramePrepArgs A) {
    const long long plane = (long long)A.oh * A.ow;
    for (int f = blockIdx.y; f < A.F; f += gridDim.y) {
        float mn = INFINITY, mx = -INFINITY;
        const uint8_t *img8 = (const uint8_t *)A.image + (long long)f * A.si_f;
        const float *img32 = (const float *)A.image + (long long)f * A.si_f;
        const float *dep = A.depth + (long long)f * A.sd_f;
        float *out = A.rgbd + (long long)f * 4 * plane;
        for (long long g = (long long)blockIdx.x * FP_THREADS + threadIdx.x; g < A.groups; g += (long long)gridDim.x * FP_THREADS) {
            const int oy = (int)(g / A.groups_x), ox0 = (int)(g - (long long)oy * A.groups_x) * FP_VEC;
            const SrcTap ty = src_tap<SMALL>(oy, A.H, A.oh);
            SrcTap tx[FP_VEC];
            for (int j = 0; j < FP_VEC; ++j) {                   // a column past the row's end repeats the last one and is not stored
                const int ox = ox0 + j < A.ow ? ox0 + j : A.ow - 1;
                tx[j] = src_tap<SMALL>(ox, A.W, A.ow);
            }
            float *row = out + (long long)oy * A.ow + ox0;
            for (int c = 0; c < 4; ++c) {
                float v[FP_VEC];
                for (int j = 0; j < FP_VEC; ++j) {
                    float a, b, cc, d;
                    if (c == 3) {
                        const float *r0 = dep + ty.i0 * A.sd_y, *r1 = dep + ty.i1 * A.sd_y;
                        a = r0[tx[j].i0 * A.sd_x]; b = r0[tx[j].i1 * A.sd_x]; cc = r1[tx[j].i0 * A.sd_x]; d = r1[tx[j].i1 * A.sd_x];
                    } else if (A.is_u8) {
                        const uint8_t *r0 = img8 + c * A.si_c + ty.i0 * A.si_y, *r1 = img8 + c * A.si_c + ty.i1 * A.si_y;
                        a = (float)r0[tx[j].i0 * A.si_x]; b = (float)r0[tx[j].i1 * A.si_x];
                        cc = (float)r1[tx[j].i0 * A.si_x]; d = (float)r1[tx[j].i1 * A.si_x];
                    } else {
                        const float *r0 = img32 + c * A.si_c + ty.i0 * A.si_y, *r1 = img32 + c * A.si_c + ty.i1 * A.si_y;
                        a = r0[tx[j].i0 * A.si_x]; b = r0[tx[j].i1 * A.si_x]; cc = r1[tx[j].i0 * A.si_x]; d = r1[tx[j].i1 * A.si_x];
                    }
                    float r = blend(a, b, cc, d, ty, tx[j]);
                    if (c < 3 && A.normalise) r = unit_colour(r);
                    v[j] = r;
                }
                float *dst = row + c * plane;
                if (A.vec) {
                    *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
                    for (int j = 0; j < FP_VEC; ++j)
                        if (ox0 + j < A.ow) dst[j] = v[j];
                }
                if (c == 3)
                    for (int j = 0; j < FP_VEC; ++j)
                        if (ox0 + j < A.ow) depth_range_fold(v[j], A.use_log, mn, mx);
            }
        }
        minmax_finish(mn, mx, A.part + (long long)f * 2 * gridDim.x, A.ticket + f, A.drange + 2 * f, blockIdx.x, gridDim.x);
    }
}

// blocks a frame (the grid's x), or 0 when the sizes are refused
static long long fp_blocks(long long oh, long long ow) {
    if (oh < 1 || ow < 1 || oh > kI31 || ow > kI31) return 0;
    const long long groups = oh * ((ow + FP_VEC - 1) / FP_VEC), nb = (groups + FP_THREADS - 1) / FP_THREADS;
    return nb < BT_VIDEO_MAX_BLOCKS ? nb : BT_VIDEO_MAX_BLOCKS;
}

static size_t fp_ticket_bytes(long long F) { return (size_t)((F + 3) / 4) * 16; }

}  // namespace bt

extern "C" size_t bt_frame_prep_workspace_bytes(int64_t F, int64_t oh, int64_t ow) {
    const long long nb = bt::fp_blocks(oh, ow);
    if (F < 1 || F > bt::kI31 || nb == 0 || (__int128)F * 4 * oh * ow > bt::kI31) return 0;
    return bt::fp_ticket_bytes(F) + (size_t)F * nb * 2 * sizeof(float);
}

extern "C" int bt_frame_prep(const void *image, int32_t image_is_u8, int64_t si_f, int64_t si_c, int64_t si_y, int64_t si_x,
                             const float *depth, int64_t sd_f, int64_t sd_y, int64_t sd_x, int64_t F, int64_t H, int64_t W, int64_t oh,
                             int64_t ow, int32_t normalise, int32_t use_log_depth, void *workspace, float *rgbd, float *drange,
                             void *stream) {
    if (!image || !depth || !workspace || !rgbd || !drange || F < 0 || H < 1 || W < 1 || oh < 1 || ow < 1) return BT_EINVAL;
    if (si_f < 0 || si_c < 0 || si_y < 0 || si_x < 0 || sd_f < 0 || sd_y < 0 || sd_x < 0) return BT_EINVAL;
    if (F > bt::kI31 || H > bt::kI31 || W > bt::kI31 || oh > bt::kI31 || ow > bt::kI31 || (__int128)F * 4 * oh * ow > bt::kI31)
        return BT_EUNSUPPORTED;
    const long long Fv = F > 0 ? F : 1;                         // the strides are judged for F == 0 as for one frame
    if (!bt::view_fits_i31(Fv, 3, H, W, si_f, si_c, si_y, si_x) || !bt::view_fits_i31(Fv, 1, H, W, sd_f, 0, sd_y, sd_x)) return BT_EUNSUPPORTED;
    if (F == 0) return BT_OK;
    const long long nb = bt::fp_blocks(oh, ow);
    bt::FramePrepArgs A;
    A.image = image; A.depth = depth;
    A.si_f = si_f; A.si_c = si_c; A.si_y = si_y; A.si_x = si_x; A.sd_f = sd_f; A.sd_y = sd_y; A.sd_x = sd_x;
    A.F = (int)F; A.H = (int)H; A.W = (int)W; A.oh = (int)oh; A.ow = (int)ow;
    A.groups_x = (int)((ow + bt::FP_VEC - 1) / bt::FP_VEC);
    A.groups = (long long)oh * A.groups_x;
    A.is_u8 = image_is_u8 ? 1 : 0; A.normalise = normalise ? 1 : 0; A.use_log = use_log_depth ? 1 : 0;
    A.vec = (ow % bt::FP_VEC == 0 && ((uintptr_t)rgbd & 15) == 0) ? 1 : 0;
    A.ticket = (unsigned *)workspace;
    A.part = (float *)((char *)workspace + bt::fp_ticket_bytes(F));
    A.rgbd = rgbd; A.drange = drange;
    const bool small = (__int128)(2 * oh + 1) * H < (1LL << 31) && (__int128)(2 * ow + 1) * W < (1LL << 31) && 2 * oh < (1 << 24) && 2 * ow < (1 << 24);
    const dim3 grid((unsigned)nb, (unsigned)(F < BT_VIDEO_GRID_FRAMES ? F : BT_VIDEO_GRID_FRAMES));
    if (small) hipLaunchKernelGGL(bt::k_frame_prep<true>, grid, dim3(bt::FP_THREADS), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(bt::k_frame_prep<false>, grid, dim3(bt::FP_THREADS), 0, (hipStream_t)stream, A);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
