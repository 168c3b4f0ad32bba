// window_fmaps.hip — the tracker's window preparation (include/batrack_window.h holds the specification): k_depth_range,
// k_window_depth, k_embed_conv, k_feat_sample.
//
// k_depth_range and k_window_depth end in a minimum and a maximum over everything they read: the two-stage reduction of
// csrc/minmax_reduce.hpp (block pairs in the workspace, a ticket, the last block reduces them), shared with k_frame_prep.
//
// k_embed_conv is the 3 x 3 convolution 191 -> 128 as an implicit GEMM on v_mfma_f32_16x16x4_f32 with the tile of
// csrc/conv_tile.hpp (stride 1, all 128 columns): K = 9 taps x 192 input channels (191 and a zero weight).
//   K-chunk  8 input channels at a time: their 18 x 10 halo tile (zero outside the map) and their 9 x 8 x 128 weights are
//            staged in LDS, 50288 bytes with the pixels' coordinates — two workgroups share a CU (180 VGPRs allow two waves a SIMD), and while one
//            stages the other multiplies.  Chunks 0 .. 15 are the encoder's channels, read from memory; chunks 16 .. 23 are the embedding,
//            COMPUTED into the same halo tile from the pixel's normalised (x, y, z), which is kept in LDS per halo pixel.
//   order    chunk, tap, group of four channels, ONE fma chain, the bias last: fixed, the same for every pixel of every
//            frame, whatever frame0 and F are.
// What it leaves on the table is in DESIGN.md.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_window.h"
#include "conv_tile.hpp"
#include "minmax_reduce.hpp"
#include "sample_taps.hpp"

namespace bt {

constexpr int WD_MAX_BLOCKS = 1024, WD_PER_THREAD = 8;         // WD_THREADS: minmax_reduce.hpp
constexpr size_t WD_WORKSPACE = (size_t)2 * WD_MAX_BLOCKS * sizeof(float) + sizeof(unsigned);

constexpr int EC_HW = ConvGeom<1>::HW, EC_HALO = ConvGeom<1>::HALO, EC_PL = ConvGeom<1>::PL;
constexpr int EC_CHUNKS = (BT_WINDOW_C + BT_WINDOW_EMB + 1) / CT_KC, EC_NT = BT_WINDOW_C / 16;
static_assert(CT_KC == BT_WINDOW_KCHUNK && EC_CHUNKS * CT_KC == 192, "the packed weights' chunks");

constexpr int FS_THREADS = BT_WINDOW_C;

// --------------------------------------------------------------------------------------------------------- k_depth_range
__global__ __launch_bounds__(WD_THREADS) void k_depth_range(const float *__restrict__ depth, int H, int W, long long st, long long sy,
                                                           long long sx, long long total, int use_log, float *part,
                                                           unsigned *ticket, float *out) {
    float mn = INFINITY, mx = -INFINITY;
    for (long long i = (long long)blockIdx.x * WD_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * WD_THREADS) {
        const long long row = i / W, t = row / H;
        const int x = (int)(i - row * W), y = (int)(row - t * H);
        const float d = depth[t * st + y * sy + x * sx];
        depth_range_fold(d, use_log, mn, mx);                    // (d > 0.01 is false for a NaN: only the log form can meet one)
    }
    minmax_finish(mn, mx, part, ticket, out, blockIdx.x, gridDim.x);
}

// -------------------------------------------------------------------------------------------------------- k_window_depth
__global__ __launch_bounds__(WD_THREADS) void k_window_depth(const float *__restrict__ depth, int frames, int h, int w, long long st,
                                                            long long sy, long long sx, int stride, float d_near, float d_range,
                                                            float Dz, int use_log, long long total, float *__restrict__ dmaps,
                                                            float *part, unsigned *ticket, float *zrange) {
    float mn = INFINITY, mx = -INFINITY;
    for (long long i = (long long)blockIdx.x * WD_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * WD_THREADS) {
        const long long row = i / w, t = row / h;
        const int x = (int)(i - row * w), y = (int)(row - t * h);
        const long long ts = t < frames ? t : frames - 1;        // a short last window repeats its last frame
        const float d = depth_process(depth[ts * st + (long long)y * stride * sy + (long long)x * stride * sx], use_log);
        const float v = __fmul_rn(__fdiv_rn(__fsub_rn(d, d_near), d_range), Dz);
        dmaps[i] = v;
        nan_minmax(v, mn, mx);
    }
    minmax_finish(mn, mx, part, ticket, zrange, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------------------------------------------------- k_embed_conv
// 2 ((v - lo) / (hi - lo) - 0.5), md_tracker.py:525-528, every operation rounded
__device__ __forceinline__ float normalise(float v, float lo, float hi) {
    return __fmul_rn(2.0f, __fsub_rn(__fdiv_rn(__fsub_rn(v, lo), __fsub_rn(hi, lo)), 0.5f));
}

__global__ __launch_bounds__(CT_THREADS) void k_embed_conv(const float *__restrict__ fnet, long long sf, long long sc, long long sy,
                                                          long long sx, const float *__restrict__ dmaps,
                                                          const float *__restrict__ zrange, const float *__restrict__ wp,
                                                          const float *__restrict__ bias, const float *__restrict__ freqs,
                                                          int frame0, int h, int w, int tiles_x, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float w_l[9 * CT_KC * conv_wld(BT_WINDOW_C)];   // [tap][channel of the chunk][144]
    __shared__ float in_l[CT_KC * EC_PL];                                         // [channel of the chunk][halo pixel]
    __shared__ float p_l[3 * EC_HALO];                                            // normalised x, y, z of the halo pixels
    const int tid = threadIdx.x;
    const int f = blockIdx.y, ty0 = (blockIdx.x / tiles_x) * CT_TH, tx0 = (blockIdx.x % tiles_x) * CT_TW;
    const long long hw = (long long)h * w;

    {
        const float zlo = zrange[0], zhi = zrange[1];
        const float *dm = dmaps + (long long)(frame0 + f) * hw;
        for (int p = tid; p < EC_HALO; p += CT_THREADS) {
            const int gy = ty0 + p / EC_HW - 1, gx = tx0 + p % EC_HW - 1;
            const bool inside = gy >= 0 && gy < h && gx >= 0 && gx < w;
            p_l[p] = normalise((float)gx, 0.0f, (float)(w - 1));
            p_l[EC_HALO + p] = normalise((float)gy, 0.0f, (float)(h - 1));
            p_l[2 * EC_HALO + p] = inside ? normalise(dm[(long long)gy * w + gx], zlo, zhi) : 0.0f;
        }
    }

    f32x4 acc[2][EC_NT];
    tile_zero<EC_NT>(acc);

    const float *fbase = fnet + (long long)f * sf;
    for (int chunk = 0; chunk < EC_CHUNKS; ++chunk) {
        __syncthreads();                                         // the previous chunk's reads are done (and p_l is written)
        tile_stage_rows<9 * CT_KC, BT_WINDOW_C>(w_l, wp + (size_t)chunk * 9 * CT_KC * BT_WINDOW_C, BT_WINDOW_C);
        for (int idx = tid; idx < CT_KC * EC_HALO; idx += CT_THREADS) {
            const int chl = idx / EC_HALO, p = idx - chl * EC_HALO;
            const int gy = ty0 + p / EC_HW - 1, gx = tx0 + p % EC_HW - 1;
            float v = 0.0f;                                      // zero padding, for the embedding as for the maps
            if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
                const int c = chunk * CT_KC + chl;
                if (c < BT_WINDOW_C) v = fbase[c * sc + gy * sy + gx * sx];
                else {
                    const int e = c - BT_WINDOW_C;               // Embedder_Fourier's order: the input, then per frequency sin(xyz), cos(xyz)
                    if (e < 3) v = p_l[e * EC_HALO + p];
                    else if (e < BT_WINDOW_EMB) {
                        const int i = (e - 3) / 6, r = (e - 3) - 6 * i;
                        const float arg = __fmul_rn(p_l[(r < 3 ? r : r - 3) * EC_HALO + p], freqs[i]);
                        v = r < 3 ? sinf(arg) : cosf(arg);
                    }
                }
            }
            in_l[chl * EC_PL + p] = v;
        }
        __syncthreads();
        tile_taps<1, EC_NT>(in_l, w_l, acc);
    }
    tile_store_stats<EC_NT, false>(acc, bias, out + (long long)f * BT_WINDOW_C * hw, hw, h, w, ty0, tx0, nullptr, nullptr);
}

// --------------------------------------------------------------------------------------------------------- k_feat_sample
// one block per query, one thread per channel; the taps are the query's, the same in every thread
__global__ __launch_bounds__(FS_THREADS) void k_feat_sample(const float *__restrict__ fmaps, int S, int h, int w,
                                                           const int *__restrict__ frames, const float *__restrict__ xy,
                                                           long long xy_stride, long long n, float *__restrict__ out) {
    const long long hw = (long long)h * w;
    for (long long k = blockIdx.x; k < n; k += gridDim.x) {
        int fr = frames[k];
        fr = fr < 0 ? 0 : (fr > S - 1 ? S - 1 : fr);
        const BilinearTaps t = bilinear_taps(h, w, xy[k * xy_stride], xy[k * xy_stride + 1]);
        out[k * BT_WINDOW_C + threadIdx.x] = bilinear_blend(fmaps + ((long long)fr * BT_WINDOW_C + threadIdx.x) * hw, t);
    }
}

static unsigned wd_blocks(long long total) {
    const long long nb = (total + (long long)WD_THREADS * WD_PER_THREAD - 1) / ((long long)WD_THREADS * WD_PER_THREAD);
    return (unsigned)(nb < 1 ? 1 : (nb < WD_MAX_BLOCKS ? nb : WD_MAX_BLOCKS));
}

// the largest element offset a [T, H, W] view with these strides reaches, or -1 when it passes 2^31 - 1
static long long view_extent(long long T, long long H, long long W, long long st, long long sy, long long sx) {
    if (st > kI31 || sy > kI31 || sx > kI31) return -1;
    const __int128 e = (__int128)(T - 1) * st + (__int128)(H - 1) * sy + (__int128)(W - 1) * sx;
    return e > kI31 ? -1 : (long long)e;
}

}  // namespace bt

extern "C" size_t bt_window_workspace_bytes(void) { return bt::WD_WORKSPACE; }

extern "C" int bt_depth_range(const float *depth, int64_t T, int64_t H, int64_t W, int64_t stride_t, int64_t stride_y, int64_t stride_x,
                              int32_t use_log_depth, void *workspace, float *out, void *stream) {
    if (!depth || !workspace || !out || T < 1 || H < 1 || W < 1 || stride_t < 0 || stride_y < 0 || stride_x < 0) return BT_EINVAL;
    if (T > bt::kI31 || H > bt::kI31 || W > bt::kI31 || (__int128)T * H * W > bt::kI31
        || bt::view_extent(T, H, W, stride_t, stride_y, stride_x) < 0) return BT_EUNSUPPORTED;
    const long long total = (long long)T * H * W;
    float *part = (float *)workspace;
    hipLaunchKernelGGL(bt::k_depth_range, dim3(bt::wd_blocks(total)), dim3(bt::WD_THREADS), 0, (hipStream_t)stream, depth, (int)H, (int)W,
                       (long long)stride_t, (long long)stride_y, (long long)stride_x, total, (int)use_log_depth, part,
                       (unsigned *)(part + 2 * bt::WD_MAX_BLOCKS), out);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

extern "C" int bt_window_depth(const float *depth, int64_t frames, int64_t S, int64_t H, int64_t W, int64_t stride_t, int64_t stride_y,
                               int64_t stride_x, int64_t stride, float d_near, float d_range, float Dz, int32_t use_log_depth,
                               void *workspace, float *dmaps, float *zrange, void *stream) {
    if (!depth || !workspace || !dmaps || !zrange || S < 1 || frames < 1 || frames > S || H < 1 || W < 1 || stride < 1
        || stride_t < 0 || stride_y < 0 || stride_x < 0) return BT_EINVAL;
    if (S > bt::kI31 || H > bt::kI31 || W > bt::kI31 || stride > bt::kI31) return BT_EUNSUPPORTED;
    const long long h = H / stride, w = W / stride;
    if (h < 1 || w < 1) return BT_EINVAL;
    if ((__int128)S * h * w > bt::kI31 || bt::view_extent(frames, H, W, stride_t, stride_y, stride_x) < 0) return BT_EUNSUPPORTED;
    const long long total = (long long)S * h * w;
    float *part = (float *)workspace;
    hipLaunchKernelGGL(bt::k_window_depth, dim3(bt::wd_blocks(total)), dim3(bt::WD_THREADS), 0, (hipStream_t)stream, depth, (int)frames,
                       (int)h, (int)w, (long long)stride_t, (long long)stride_y, (long long)stride_x, (int)stride, d_near, d_range, Dz,
                       (int)use_log_depth, total, dmaps, part, (unsigned *)(part + 2 * bt::WD_MAX_BLOCKS), zrange);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

extern "C" int bt_embed_conv(const float *fnet, int64_t sf, int64_t sc, int64_t sy, int64_t sx, const float *dmaps, const float *zrange,
                             const float *wpacked, const float *bias, const float *freqs, int64_t S, int64_t frame0, int64_t F,
                             int64_t h, int64_t w, int64_t C, float *out, void *stream) {
    if (!fnet || !dmaps || !zrange || !wpacked || !bias || !freqs || !out || ((uintptr_t)wpacked & 15)) return BT_EINVAL;
    if (S < 1 || F < 0 || frame0 < 0 || frame0 > S || F > S - frame0 || h < 2 || w < 2 || C < 1 || sf < 0 || sc < 0 || sy < 0 || sx < 0)
        return BT_EINVAL;
    if (C != BT_WINDOW_C || S > bt::kI31 || h > bt::kI31 || w > bt::kI31 || (__int128)S * C * h * w > bt::kI31) return BT_EUNSUPPORTED;
    if (F == 0) return BT_OK;
    if (!bt::view_fits_i31(F, C, h, w, sf, sc, sy, sx)) return BT_EUNSUPPORTED;
    const long long tiles_x = bt::conv_tiles_x(w);
    if (F > 65535) return BT_EUNSUPPORTED;                       // the grid's second dimension
    hipLaunchKernelGGL(bt::k_embed_conv, dim3((unsigned)bt::conv_tiles(h, w), (unsigned)F), dim3(bt::CT_THREADS), 0, (hipStream_t)stream,
                       fnet, (long long)sf, (long long)sc, (long long)sy, (long long)sx, dmaps, zrange, wpacked, bias, freqs, (int)frame0,
                       (int)h, (int)w, (int)tiles_x, out);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

extern "C" int bt_feat_sample(const float *fmaps, int64_t S, int64_t C, int64_t h, int64_t w, const int32_t *frames, const float *xy,
                              int64_t xy_stride, int64_t n, float *out, void *stream) {
    if (!fmaps || !frames || !xy || !out || S < 1 || C < 1 || h < 1 || w < 1 || xy_stride < 2 || n < 0) return BT_EINVAL;
    if (C != BT_WINDOW_C || S > bt::kI31 || h > bt::kI31 || w > bt::kI31 || (__int128)S * C * h * w > bt::kI31 || xy_stride > bt::kI31
        || (__int128)n * C > bt::kI31 || (__int128)n * xy_stride > bt::kI31) return BT_EUNSUPPORTED;
    if (n == 0) return BT_OK;
    hipLaunchKernelGGL(bt::k_feat_sample, dim3((unsigned)(n < (1 << 20) ? n : (1 << 20))), dim3(bt::FS_THREADS), 0, (hipStream_t)stream,
                       fmaps, (int)S, (int)h, (int)w, frames, xy, (long long)xy_stride, (long long)n, out);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
