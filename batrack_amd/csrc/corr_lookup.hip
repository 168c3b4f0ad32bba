// corr_lookup.hip — the tracker's CorrBlock (corr + sample) without the correlation volume, for gfx950
// (specification: include/batrack_corr.h; the reference: main/frontend/core/cotracker/blocks.py:326-385).
//
// k_corr_pyramid / k_corr_pyramid_pool, once per CorrBlock: the feature maps channels-last, every level, in one packed
// buffer, so that the feature row of a pixel is 4*C contiguous bytes and the rows of neighbouring x are adjacent.
// k_corr_lookup*, once per sample(): one wave takes one (frame, query, level).  It needs the (2r+2)^2 integer positions
// around the window once (all fractional offsets inside a window are equal): gather their rows, dot each with the
// query's target vector, blend four neighbours to each of the (2r+1)^2 outputs.  Positions outside the map are
// predicated off (never read, exactly 0).  No atomics, no workspace; fixed summation order: a call repeats bit for bit.
//
// The tuned case, C = 128 and r = 3, has 64 positions — one wavefront — and two lane layouts (DESIGN.md has the numbers):
//   channels: 32 lanes x 16 B across a row, two rows a wave-instruction, 32 instructions; the eight x-neighbours of a
//             window row are 4 KB contiguous.  Each lane ends with 32 partial sums, one per instruction; they are folded
//             while they are reduced (31 cross-lane adds instead of 32 x 5), after which lane j of half h holds the
//             whole dot product of position 2j + h.
//   position: lane = position, each lane walks its own row in 16-B pieces against a wave-uniform target; no reduction.
// Both blend through cross-lane reads: no LDS, waves independent.  Everything else takes k_corr_lookup_any: 16 lanes a
// row, four rows a step, dots through LDS.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_corr.h"

namespace bt {

struct CorrLevels {                 // by value to the kernels
    int H[BT_CORR_MAX_LEVELS], W[BT_CORR_MAX_LEVELS];
    long long off[BT_CORR_MAX_LEVELS];      // first float of level l in the packed pyramid
    long long total;                        // floats in all levels
};

// levels of a valid (S, C, H, W, L); false when a level would be empty
static bool corr_levels(int64_t S, int64_t C, int64_t H, int64_t W, int L, CorrLevels *lv) {
    long long off = 0;
    for (int l = 0; l < L; ++l) {
        if (H < 1 || W < 1) return false;
        lv->H[l] = (int)H; lv->W[l] = (int)W; lv->off[l] = off;
        off += (long long)S * H * W * C;
        H /= 2; W /= 2;
    }
    lv->total = off;
    return true;
}

constexpr int CL_THREADS = 256, CL_WAVES = CL_THREADS / 64;

// ---- pyramid ---------------------------------------------------------------------------------------------------------

// level 0: [S', C, HW] -> [S', HW, C], tiles of 32 channels x 64 pixels through LDS (256-B reads, 128-B writes)
__global__ __launch_bounds__(CL_THREADS) void k_corr_pyramid(const float *__restrict__ fmaps, float *__restrict__ out, int C, int HW,
                                                              int tiles_hw, int tiles_c, long long ntiles) {
    __shared__ float tile[32][65];
    const int tid = threadIdx.x;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tp = (int)(t % tiles_hw);
        const long long q = t / tiles_hw;
        const int tc = (int)(q % tiles_c);
        const long long s = q / tiles_c;
        const int p0 = tp * 64, c0 = tc * 32;
        const float *src = fmaps + (size_t)s * C * HW;
        float *dst = out + (size_t)s * HW * C;
        const int px = tid & 63, cr = tid >> 6;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = cr + 4 * k;
            if (c0 + c < C && p0 + px < HW) tile[c][px] = src[(size_t)(c0 + c) * HW + p0 + px];
        }
        __syncthreads();
        const int cc = tid & 31, pr = tid >> 5;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int p = pr + 8 * k;
            if (c0 + cc < C && p0 + p < HW) dst[(size_t)(p0 + p) * C + c0 + cc] = tile[cc][p];
        }
        __syncthreads();
    }
}

// level l+1 from level l, both channels-last: ((a + b) + c + d) / 4 over the 2 x 2 block, 16 B a lane
__global__ __launch_bounds__(CL_THREADS) void k_corr_pyramid_pool(const float4 *__restrict__ in, float4 *__restrict__ out, int C4,
                                                                   int Hi, int Wi, int Ho, int Wo, long long total) {
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < total; n += (long long)gridDim.x * blockDim.x) {
        long long q = n;
        const int c = (int)(q % C4); q /= C4;
        const int x = (int)(q % Wo); q /= Wo;
        const int y = (int)(q % Ho);
        const long long s = q / Ho;
        const float4 *r0 = in + (((size_t)s * Hi + 2 * y) * Wi + 2 * x) * C4 + c, *r1 = r0 + (size_t)Wi * C4;
        const float4 a = r0[0], b = r0[C4], e = r1[0], f = r1[C4];
        out[n] = make_float4((((a.x + b.x) + e.x) + f.x) * 0.25f, (((a.y + b.y) + e.y) + f.y) * 0.25f,
                             (((a.z + b.z) + e.z) + f.z) * 0.25f, (((a.w + b.w) + e.w) + f.w) * 0.25f);
    }
}

// ---- lookup ----------------------------------------------------------------------------------------------------------

struct CorrWin { float fx, fy; int x0, y0; };

// the window of pair `k` at a level: coords / 2^l (exact), its floor and fraction.  The integer part is clamped far
// outside any map (H, W <= 32768), so that the position arithmetic cannot overflow for any float.
__device__ __forceinline__ CorrWin corr_window(const float *__restrict__ coords, long long k, long long stride, int level) {
    const float inv = __int_as_float((127 - level) << 23);                       // 2^-level
    const float cx = coords[k * stride] * inv, cy = coords[k * stride + 1] * inv;
    const float xf = floorf(cx), yf = floorf(cy);
    CorrWin w;
    w.fx = cx - xf; w.fy = cy - yf;
    w.x0 = (int)fminf(fmaxf(xf, -1.0e6f), 1.0e6f);
    w.y0 = (int)fminf(fmaxf(yf, -1.0e6f), 1.0e6f);
    return w;
}

__device__ __forceinline__ float corr_blend(const CorrWin &w, float v00, float v01, float v10, float v11) {
    const float gx = 1.0f - w.fx, gy = 1.0f - w.fy;
    return (gx * gy) * v00 + (w.fx * gy) * v01 + (gx * w.fy) * v10 + (w.fx * w.fy) * v11;
}

__device__ __forceinline__ float corr_dot4(float4 v, float4 t, float acc) {
    return fmaf(v.w, t.w, fmaf(v.z, t.z, fmaf(v.y, t.y, fmaf(v.x, t.x, acc))));
}

// Fold and reduce 2 * O values over the lanes that differ in the bits below 2 * O: after the step with offset O a lane
// keeps the O values whose index has bit O as its own lane number has, each now summed over the pair; then the same with
// O / 2.  corr_fold<16> leaves in v[0] of lane j the sum over the 32 lanes of its half of their v[j]: 31 cross-lane adds.
// (A template, not a loop over O: the indices must be compile-time constants for v[] to stay in registers.)
template <int O>
__device__ __forceinline__ void corr_fold(float (&v)[32], int j) {
    const bool up = (j & O) != 0;
#pragma unroll
    for (int k = 0; k < O; ++k) {
        const float send = up ? v[k] : v[k + O], keep = up ? v[k + O] : v[k];
        v[k] = keep + __shfl_xor(send, O);
    }
    if constexpr (O > 1) corr_fold<O / 2>(v, j);
}

// C = 128, r = 3.  LAYOUT 0: lanes across channels, 1: lane = position (see the head of the file).
template <int LAYOUT>
__global__ __launch_bounds__(CL_THREADS) void k_corr_lookup(const float *__restrict__ pyr, const CorrLevels lv, int L,
                                                             const float *__restrict__ targets, const float *__restrict__ coords,
                                                             long long cstride, long long items, long long N, float sqrt_c,
                                                             float *__restrict__ out) {
    constexpr int C = 128, R = 3, D = 2 * R + 2, d = 2 * R + 1;
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * CL_WAVES + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * CL_WAVES;
    for (long long it = wave0; it < items; it += nwaves) {
        const unsigned item = (unsigned)__builtin_amdgcn_readfirstlane((int)it);          // wave-uniform, and known to be
        const int l = (int)(item % (unsigned)L);
        const unsigned sn = item / (unsigned)L, s = sn / (unsigned)N;
        const CorrWin w = corr_window(coords, sn, cstride, l);
        const int Hl = lv.H[l], Wl = lv.W[l];
        const float *base = pyr + lv.off[l] + (size_t)s * Hl * Wl * C;
        const float *tg = targets + (size_t)sn * C;
        float dot;                                  // this lane's position: src_lane() says which
        if (LAYOUT == 0) {
            const int h = lane >> 5, j = lane & 31;
            const float4 t = reinterpret_cast<const float4 *>(tg)[j];
            float v[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) {          // positions 2i + h: window row i / 4, columns 2 (i % 4) + h
                const int y = w.y0 - R + (i >> 2), x = w.x0 - R + 2 * (i & 3) + h;
                const bool ok = y >= 0 && y < Hl && x >= 0 && x < Wl;
                // a branch per row would make the wave wait for every load before it issues the next: a lane whose
                // position is outside the map reads its piece of the target instead (never the map) and keeps 0
                const float4 *row = ok ? reinterpret_cast<const float4 *>(base + ((size_t)y * Wl + x) * C) : reinterpret_cast<const float4 *>(tg);
                const float part = corr_dot4(row[j], t, 0.0f);
                v[i] = ok ? part : 0.0f;
            }
            corr_fold<16>(v, j);
            dot = v[0] / sqrt_c;                    // position 2j + h
        } else {
            const int y = w.y0 - R + (lane >> 3), x = w.x0 - R + (lane & 7);
            const bool ok = y >= 0 && y < Hl && x >= 0 && x < Wl;
            float acc = 0.0f;
            if (ok) {
                // 16 interleaved partial sums (channel c goes to sum c % 16), added pairwise: one chain of 128 fused
                // multiply-adds rounds three times as far from the exact dot product as the other kernels' sums do
                const float4 *row = reinterpret_cast<const float4 *>(base + ((size_t)y * Wl + x) * C);
                const float4 *t4 = reinterpret_cast<const float4 *>(tg);
                float a[16] = {};
#pragma unroll 2
                for (int c = 0; c < C / 4; c += 4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float4 v = row[c + u], t = t4[c + u];
                        a[4 * u + 0] = fmaf(v.x, t.x, a[4 * u + 0]);
                        a[4 * u + 1] = fmaf(v.y, t.y, a[4 * u + 1]);
                        a[4 * u + 2] = fmaf(v.z, t.z, a[4 * u + 2]);
                        a[4 * u + 3] = fmaf(v.w, t.w, a[4 * u + 3]);
                    }
                }
#pragma unroll
                for (int o = 8; o >= 1; o >>= 1)
#pragma unroll
                    for (int k = 0; k < o; ++k) a[k] += a[k + o];
                acc = a[0];
            }
            dot = acc / sqrt_c;                     // position = lane
        }
        // blend: output o = a * d + b reads positions (b, a), (b, a+1), (b+1, a), (b+1, a+1) of the D x D grid
        const int o = lane < d * d ? lane : 0, a = o / d, b = o % d, p = b * D + a;
        auto src_lane = [](int pos) { return LAYOUT == 0 ? (pos >> 1) | ((pos & 1) << 5) : pos; };
        const float v00 = __shfl(dot, src_lane(p)), v01 = __shfl(dot, src_lane(p + 1));
        const float v10 = __shfl(dot, src_lane(p + D)), v11 = __shfl(dot, src_lane(p + D + 1));
        if (lane < d * d) out[(size_t)item * (d * d) + lane] = corr_blend(w, v00, v01, v10, v11);
    }
}

// any C % 4 == 0 up to 512, r <= 7 (256 positions), L <= 8: 16 lanes a row, four rows a step, dots through LDS
__global__ __launch_bounds__(CL_THREADS) void k_corr_lookup_any(const float *__restrict__ pyr, const CorrLevels lv, int C, int L, int R,
                                                                 const float *__restrict__ targets, const float *__restrict__ coords,
                                                                 long long cstride, long long items, long long N, float sqrt_c,
                                                                 float *__restrict__ out) {
    __shared__ float s_dot[CL_WAVES][4 * (BT_CORR_MAX_RADIUS + 1) * (BT_CORR_MAX_RADIUS + 1)];
    __shared__ float4 s_tgt[CL_WAVES][BT_CORR_MAX_CHANNELS / 4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const int D = 2 * R + 2, d = 2 * R + 1, P = D * D, C4 = C / 4;     // P is a multiple of 4
    const long long nblk = (items + CL_WAVES - 1) / CL_WAVES;
    for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {   // block-uniform trip count: barriers inside
        const long long item = blk * CL_WAVES + wave;
        const bool on = item < items;
        const int l = __builtin_amdgcn_readfirstlane(on ? (int)((unsigned)item % (unsigned)L) : 0);   // one item a wave: uniform, and known to be
        const unsigned sn = on ? (unsigned)item / (unsigned)L : 0, s = sn / (unsigned)N;
        if (on) {
            const float4 *tg = reinterpret_cast<const float4 *>(targets + (size_t)sn * C);
            for (int c = lane; c < C4; c += 64) s_tgt[wave][c] = tg[c];
        }
        __syncthreads();
        const CorrWin w = corr_window(coords, sn, cstride, l);
        const int Hl = lv.H[l], Wl = lv.W[l];
        const float *base = pyr + lv.off[l] + (size_t)s * Hl * Wl * C;
        if (on) {
            for (int p0 = 0; p0 < P; p0 += 4) {
                const int p = p0 + g, y = w.y0 - R + p / D, x = w.x0 - R + p % D;
                const bool ok = y >= 0 && y < Hl && x >= 0 && x < Wl;
                float acc = 0.0f;
                if (ok) {
                    const float4 *row = reinterpret_cast<const float4 *>(base + ((size_t)y * Wl + x) * C);
                    for (int c = j; c < C4; c += 16) acc = corr_dot4(row[c], s_tgt[wave][c], acc);
                }
                acc += __shfl_xor(acc, 8);
                acc += __shfl_xor(acc, 4);
                acc += __shfl_xor(acc, 2);
                acc += __shfl_xor(acc, 1);
                if (j == 0) s_dot[wave][p] = acc / sqrt_c;
            }
        }
        __syncthreads();
        if (on) {
            const float *dt = s_dot[wave];
            for (int o = lane; o < d * d; o += 64) {
                const int a = o / d, b = o % d, p = b * D + a;
                out[(size_t)item * (d * d) + o] = corr_blend(w, dt[p], dt[p + 1], dt[p + D], dt[p + D + 1]);
            }
        }
        __syncthreads();
    }
}

static int g_corr_layout = 0;

// argument checks shared by the three entry points: BT_OK, BT_EINVAL or BT_EUNSUPPORTED
static int corr_check(int64_t S, int64_t C, int64_t H, int64_t W, int32_t levels, CorrLevels *lv) {
    if (S < 1 || C < 1 || H < 1 || W < 1 || levels < 1 || C % 4 != 0) return BT_EINVAL;
    if (C > BT_CORR_MAX_CHANNELS || levels > BT_CORR_MAX_LEVELS || H > 32768 || W > 32768) return BT_EUNSUPPORTED;
    if (!corr_levels(S, C, H, W, levels, lv)) return BT_EINVAL;
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_config_corr_lookup_layout(int32_t layout) {
    const int prev = bt::g_corr_layout;
    if (layout >= 0 && layout <= 2) bt::g_corr_layout = layout;
    return prev;
}

extern "C" size_t bt_corr_pyramid_bytes(int64_t S, int64_t C, int64_t H, int64_t W, int32_t levels) {
    bt::CorrLevels lv;
    return bt::corr_check(S, C, H, W, levels, &lv) == BT_OK ? (size_t)lv.total * sizeof(float) : 0;
}

extern "C" int bt_corr_pyramid(const float *fmaps, int64_t S, int64_t C, int64_t H, int64_t W, int32_t levels,
                               float *pyramid, void *stream) {
    bt::CorrLevels lv;
    if (!fmaps || !pyramid) return BT_EINVAL;
    if (const int rc = bt::corr_check(S, C, H, W, levels, &lv)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int HW = (int)(H * W), tiles_hw = (HW + 63) / 64, tiles_c = (int)((C + 31) / 32);
    const long long ntiles = (long long)S * tiles_c * tiles_hw;
    hipLaunchKernelGGL(bt::k_corr_pyramid, dim3((unsigned)(ntiles < 8192 ? ntiles : 8192)), dim3(bt::CL_THREADS), 0, st,
                       fmaps, pyramid, (int)C, HW, tiles_hw, tiles_c, ntiles);
    for (int l = 1; l < levels; ++l) {
        const long long total = (long long)S * lv.H[l] * lv.W[l] * (C / 4), nb = (total + bt::CL_THREADS - 1) / bt::CL_THREADS;
        hipLaunchKernelGGL(bt::k_corr_pyramid_pool, dim3((unsigned)(nb < 8192 ? nb : 8192)), dim3(bt::CL_THREADS), 0, st,
                           reinterpret_cast<const float4 *>(pyramid + lv.off[l - 1]), reinterpret_cast<float4 *>(pyramid + lv.off[l]),
                           (int)(C / 4), lv.H[l - 1], lv.W[l - 1], lv.H[l], lv.W[l], total);
    }
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

extern "C" int bt_corr_lookup(const float *pyramid, int64_t S, int64_t C, int64_t H, int64_t W, int32_t levels, int32_t radius,
                              const float *targets, const float *coords, int64_t coord_stride, int64_t N, float *out,
                              void *stream) {
    bt::CorrLevels lv;
    if (!pyramid || !targets || !coords || !out || N < 0 || radius < 0 || coord_stride < 2) return BT_EINVAL;
    if (const int rc = bt::corr_check(S, C, H, W, levels, &lv)) return rc;
    if (radius > BT_CORR_MAX_RADIUS) return BT_EUNSUPPORTED;
    if (N == 0) return BT_OK;
    if (N > (int64_t)0x7fffffff / (S * levels)) return BT_EUNSUPPORTED;           // S * N * L work items: 32-bit index arithmetic in the kernels
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long items = (long long)S * N * levels;
    long long nb = (items + bt::CL_WAVES - 1) / bt::CL_WAVES;
    if (nb > 2048) nb = 2048;                      // 256 CUs x 8 resident workgroups; the kernels stride over the rest
    const float sqrt_c = std::sqrt((float)C);
    const dim3 grid((unsigned)nb), block(bt::CL_THREADS);
    if (C == 128 && radius == 3 && bt::g_corr_layout == 0)
        hipLaunchKernelGGL(bt::k_corr_lookup<0>, grid, block, 0, st, pyramid, lv, (int)levels, targets, coords,
                           (long long)coord_stride, items, (long long)N, sqrt_c, out);
    else if (C == 128 && radius == 3 && bt::g_corr_layout == 1)
        hipLaunchKernelGGL(bt::k_corr_lookup<1>, grid, block, 0, st, pyramid, lv, (int)levels, targets, coords,
                           (long long)coord_stride, items, (long long)N, sqrt_c, out);
    else
        hipLaunchKernelGGL(bt::k_corr_lookup_any, grid, block, 0, st, pyramid, lv, (int)C, (int)levels, (int)radius, targets, coords,
                           (long long)coord_stride, items, (long long)N, sqrt_c, out);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
