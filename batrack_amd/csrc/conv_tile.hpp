// conv_tile.hpp — what the implicit-GEMM convolution kernels on v_mfma_f32_16x16x4_f32 share after their K loop (k_res_conv in
// csrc/encoder_trunk.hip; k_head_conv and k_embed_conv carry their own copies of the same statements, and moving them here
// is a refactor of its own that has to be shown bit-neutral).
//
// The tile.  A workgroup of 4 waves owns a 16 x 8 tile of output pixels of one frame and 16 NT output columns; wave v owns
// tile rows 2v and 2v + 1, each a 16-pixel MFMA row block: 2 x NT accumulators of 4 registers.  Register j of lane l is pixel
// 4 (l / 16) + j of the row block, column 16 ct + l % 16.
//
// tile_flush         tot += acc, acc = 0: one rounded float32 add per element.  The MFMA is a float32 fma chain; the callers
//                    end a chain every CT_FLUSH = 2 chunks of 8 channels x 9 taps (144 products).
// tile_store_stats   raw = fl(tot + bias[column]) stored as [column][h * w] planes for the pixels inside the h x w map, and
//                    per column the float64 sum and sum of squares of the float32 values STORED: lane (row block 0 then 1,
//                    j ascending), then __shfl_xor 16 and 32, then the four waves in wave order through LDS; written as
//                    part_tile[column][2].  No atomics, and every (frame, tile, column) pair is written by its workgroup: the
//                    partials need no initialisation.  Contains barriers: every thread of the workgroup calls it, and `red`
//                    (LDS, 4 * 16 NT * 2 doubles) must not be in use by a thread that has not passed a barrier.
// tile_order_stats   the partials of one (frame, column) added in tile order; mean = sum / n, var = max(sumsq / n - mean^2, 0),
//                    rstd = 1 / sqrt(var + 1e-5), all float64, returned as floats.  A constant channel has an exact mean.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace bt {

typedef float ct_f32x4 __attribute__((ext_vector_type(4)));

constexpr int CT_THREADS = 256, CT_TW = 16, CT_TH = 8, CT_KC = 8, CT_FLUSH = 2;
static_assert(CT_TH == 2 * (CT_THREADS / 64), "a wave owns two tile rows");

template <int NT>
__device__ __forceinline__ void tile_flush(ct_f32x4 (&tot)[2][NT], ct_f32x4 (&acc)[2][NT]) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            tot[r][ct] += acc[r][ct];
            acc[r][ct] = ct_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
}

template <int NT>
__device__ __forceinline__ void tile_store_stats(const ct_f32x4 (&tot)[2][NT], const float *__restrict__ bias, float *__restrict__ planes,
                                                 long long hw, int h, int w, int ty0, int tx0, double *red, double *__restrict__ part_tile) {
    constexpr int COLS = 16 * NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
        const int col = ct * 16 + l16;
        const float b = bias[col];
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = ty0 + 2 * wave + r;
            float *yrow = planes + (long long)col * hw + (long long)y * w;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = tx0 + 4 * q + j;
                if (y < h && x < w) {
                    const float v = __fadd_rn(tot[r][ct][j], b);
                    yrow[x] = v;
                    s1 += (double)v;
                    s2 += (double)v * (double)v;
                }
            }
        }
        s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
        s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
        if (q == 0) { red[(wave * COLS + col) * 2] = s1; red[(wave * COLS + col) * 2 + 1] = s2; }
    }
    __syncthreads();
    if (tid < COLS) {
        double s1 = red[tid * 2], s2 = red[tid * 2 + 1];
        for (int v = 1; v < CT_THREADS / 64; ++v) { s1 += red[(v * COLS + tid) * 2]; s2 += red[(v * COLS + tid) * 2 + 1]; }
        part_tile[tid * 2] = s1; part_tile[tid * 2 + 1] = s2;
    }
    __syncthreads();
}

// pp: the first tile's [sum, sum of squares] of this (frame, column), 16-byte aligned; `stride` doubles (even) from one tile's to the next
__device__ __forceinline__ void tile_order_stats(const double *__restrict__ pp, long long stride, int tiles, double n, float &mean_out, float &rstd_out) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 16
    for (int t = 0; t < tiles; ++t) {                            // 16 loads in flight; the adds stay in tile order
        const double2 v = *reinterpret_cast<const double2 *>(pp + t * stride);
        s1 += v.x; s2 += v.y;
    }
    const double mean = s1 / n;
    double var = s2 / n - mean * mean;
    var = var > 0.0 ? var : 0.0;
    mean_out = (float)mean;
    rstd_out = (float)(1.0 / sqrt(var + 1e-5));
}

}  // namespace bt
