// rows_linear.hip — bt_rows_linear (include/batrack_rows.h, which holds the specification): the row-wise parts of the update
// transformers, out = residual + act((pro(x) . W^T) / s + bias), as one launch on v_mfma_f32_16x16x32_f16 with float32 operands
// split into f16 pairs (hi + lo) and three products a K step, accumulated in float32.
//
// A workgroup of 256 threads (4 waves, 2 x 2) owns a 128 x 128 tile of out, 64 x 64 a wave as 4 x 4 MFMA tiles of 16 x 16
// (64 accumulator registers).  Per K step of 32 the A tile (activations, split here, after the prologue) and the B tile (the
// pre-split weights) stand in LDS as hi and lo f16, rows of 32 halves padded to 40 (80 bytes: the 16 rows of a 16-lane group
// of ds_read_b128 fall on 16 distinct slots of four banks); the next step's global loads are issued before the MFMAs of the
// current one and held in registers.  Both fragments of the MFMA are 8 consecutive k of one row (lane l: row l & 15,
// k = 8 (l >> 4) + j), and x and W are both K-contiguous, so nothing is transposed.
// With the LayerNorm prologue every workgroup first takes the statistics of its 128 rows (a quarter wave a row, two passes).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/batrack_rows.h"
#include "../../include/batrack_ba.h"

namespace bt {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int RL_T = BT_ROWS_TILE;       // 128
constexpr int RL_KS = BT_ROWS_KSTEP;     // 32
constexpr int RL_LD = RL_KS + 8;         // halves a row in LDS

template <bool VEC>
__device__ __forceinline__ void load8f(const float *p, float (&v)[8]) {
    if (VEC) {
        const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[i];
    }
}

template <bool VEC>
__device__ __forceinline__ float4 load4f(const float *p) {
    if (VEC) return *reinterpret_cast<const float4 *>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

// 8 consecutive f16 of a weight row, as their 16 bytes
template <bool VEC>
__device__ __forceinline__ uint4 load8h(const unsigned short *p) {
    if (VEC) return *reinterpret_cast<const uint4 *>(p);
    uint4 r;
    r.x = (unsigned)p[0] | ((unsigned)p[1] << 16);
    r.y = (unsigned)p[2] | ((unsigned)p[3] << 16);
    r.z = (unsigned)p[4] | ((unsigned)p[5] << 16);
    r.w = (unsigned)p[6] | ((unsigned)p[7] << 16);
    return r;
}

__device__ __forceinline__ float clamp_h(float v) {          // NaN passes through both comparisons
    return v > 65504.f ? 65504.f : (v < -65504.f ? -65504.f : v);
}

__device__ __forceinline__ float gelu_tanh(float v) {
    return 0.5f * v * (1.f + tanhf(0.7978845608028654f * (v + 0.044715f * v * v * v)));
}

// 16 partial sums of a row, one a lane of a quarter wave -> their sum in every lane of the quarter
__device__ __forceinline__ float quarter_sum(float s) {
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    return s;
}

template <bool VEC, bool X3>
__global__ __launch_bounds__(256, 2) void k_rows_linear(const float *__restrict__ x, long long ldx, const unsigned short *__restrict__ w_hi,
                                                         const unsigned short *__restrict__ w_lo, float inv_scale,
                                                         const float *__restrict__ bias, const float *residual, long long ldr, float *out,
                                                         long long ldo, int rows, int K, int Nout, int n_ct, int layernorm, float eps, int act) {
    __shared__ __attribute__((aligned(16))) _Float16 a_hi[RL_T * RL_LD];
    __shared__ __attribute__((aligned(16))) _Float16 a_lo[RL_T * RL_LD];
    __shared__ __attribute__((aligned(16))) _Float16 b_hi[RL_T * RL_LD];
    __shared__ __attribute__((aligned(16))) _Float16 b_lo[RL_T * RL_LD];
    __shared__ float s_mean[RL_T], s_rstd[RL_T];
    __shared__ int s_sat[2];                      // K step parity -> has the step's A tile an activation that saturates hi

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int r0 = (int)(blockIdx.x / (unsigned)n_ct) * RL_T, c0 = (int)(blockIdx.x % (unsigned)n_ct) * RL_T;   // < 2^31: the host checked

    if (tid < 2) s_sat[tid] = 0;

    // ---- LayerNorm statistics of the tile's rows: wave w takes rows 32 w .. 32 w + 31, four at a time, eight groups in flight
    if (layernorm) {
        const int chunks = K >> 2;
        float s[8], mean[8];
        const float *xr[8];
        bool ok[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int r = r0 + wave * 32 + it * 4 + g;
            ok[it] = r < rows;
            xr[it] = x + (long long)(ok[it] ? r : 0) * ldx;
            s[it] = 0.f;
        }
        for (int c = l15; c < chunks; c += 16) {
#pragma unroll
            for (int it = 0; it < 8; ++it)
                if (ok[it]) {
                    const float4 v = load4f<VEC>(xr[it] + 4 * c);
                    s[it] = (((s[it] + v.x) + v.y) + v.z) + v.w;
                }
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            mean[it] = quarter_sum(s[it]) / (float)K;
            s[it] = 0.f;
        }
        for (int c = l15; c < chunks; c += 16) {
#pragma unroll
            for (int it = 0; it < 8; ++it)
                if (ok[it]) {
                    const float4 v = load4f<VEC>(xr[it] + 4 * c);
                    const float d0 = v.x - mean[it], d1 = v.y - mean[it], d2 = v.z - mean[it], d3 = v.w - mean[it];
                    s[it] = fmaf(d3, d3, fmaf(d2, d2, fmaf(d1, d1, fmaf(d0, d0, s[it]))));
                }
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const float var = quarter_sum(s[it]) / (float)K;
            if (l15 == 0) {
                s_mean[wave * 32 + it * 4 + g] = mean[it];
                s_rstd[wave * 32 + it * 4 + g] = 1.f / sqrtf(var + eps);
            }
        }
    }
    __syncthreads();                              // the statistics and the cleared flags, before the first staging

    // ---- staging: unit u = tid + 256 i (i = 0, 1) is 8 consecutive k of tile row u >> 2 (= tid / 4 + 64 i), k = 8 (u & 3)
    const int srow = tid >> 2, sk = (tid & 3) * 8;
    float mu[2], rs[2];
    bool a_ok[2], b_ok[2];
    const float *xa[2];
    const unsigned short *wh[2], *wl[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = srow + 64 * i;
        a_ok[i] = r0 + row < rows;
        b_ok[i] = c0 + row < Nout;
        xa[i] = x + (long long)(a_ok[i] ? r0 + row : 0) * ldx + sk;
        const long long wo = (long long)(b_ok[i] ? c0 + row : 0) * K + sk;
        wh[i] = w_hi + wo;
        wl[i] = w_lo + wo;
        mu[i] = layernorm ? s_mean[row] : 0.f;
        rs[i] = layernorm ? s_rstd[row] : 1.f;
    }
    float av[2][8];
    uint4 bh[2], bl[2];
    auto fetch = [&](int k0) {
        const bool k_ok = k0 + sk < K;              // K % 8 == 0: a unit lies inside K or past it
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (a_ok[i] && k_ok) load8f<VEC>(xa[i] + k0, av[i]);
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) av[i][e] = 0.f;
            }
            if (b_ok[i] && k_ok) {
                bh[i] = load8h<VEC>(wh[i] + k0);
                if (X3) bl[i] = load8h<VEC>(wl[i] + k0);
            } else {
                bh[i] = make_uint4(0, 0, 0, 0);
                if (X3) bl[i] = make_uint4(0, 0, 0, 0);
            }
        }
    };
    auto stage = [&](int k0) {
        const bool k_ok = k0 + sk < K;
        bool sat = false;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int o = (srow + 64 * i) * RL_LD + sk;
            h8 hi, lo;
            const bool live = a_ok[i] && k_ok;      // the tails stay zero: the prologue of a zero is not zero
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = av[i][e];
                if (layernorm) v = (v - mu[i]) * rs[i];
                if (!live) v = 0.f;
                const _Float16 h = (_Float16)clamp_h(v);
                sat |= fabsf(v) > 65488.f;          // the values whose hi is +-65504 (65488 itself is a tie and rounds to 65472)
                hi[e] = h;
                lo[e] = (_Float16)clamp_h(v - (float)h);
            }
            *reinterpret_cast<h8 *>(a_hi + o) = hi;
            *reinterpret_cast<uint4 *>(b_hi + o) = bh[i];
            if (X3) {
                *reinterpret_cast<h8 *>(a_lo + o) = lo;
                *reinterpret_cast<uint4 *>(b_lo + o) = bl[i];
            }
        }
        if (X3 && sat) s_sat[(k0 / RL_KS) & 1] = 1;   // plain stores of the same value
    };

    const int wm = wave >> 1, wn = wave & 1;
    f4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    const int fa = (wm * 64 + l15) * RL_LD + g * 8, fb = (wn * 64 + l15) * RL_LD + g * 8;
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += RL_KS) {
        stage(k0);
        __syncthreads();
        if (k0 + RL_KS < K) fetch(k0 + RL_KS);
        h8 ah[4], bhf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ah[i] = *reinterpret_cast<const h8 *>(a_hi + fa + i * 16 * RL_LD);
            bhf[i] = *reinterpret_cast<const h8 *>(b_hi + fb + i * 16 * RL_LD);
        }
        // one accumulator; an element's order is hi.hi, hi.lo, lo.hi in every K step.  The term is the outer loop, so that
        // sixteen independent MFMAs stand between two on the same accumulator.
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bhf[j], acc[i][j], 0, 0, 0);
        if (X3) {
            h8 lof[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) lof[i] = *reinterpret_cast<const h8 *>(b_lo + fb + i * 16 * RL_LD);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], lof[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) lof[i] = *reinterpret_cast<const h8 *>(a_lo + fa + i * 16 * RL_LD);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(lof[i], bhf[j], acc[i][j], 0, 0, 0);
            // Where hi saturates (|a| > 65488) lo is no longer small against it, and neither is lo.lo against the sum: a
            // fourth product adds it for those activations alone.  Every other activation enters it as an exact zero, so
            // the step may be skipped (a workgroup-uniform branch) whenever the tile holds none, without a row's bits
            // depending on its neighbours.
            const int par = (k0 / RL_KS) & 1;
            if (s_sat[par]) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const _Float16 m = ah[i][e] < (_Float16)0.f ? -ah[i][e] : ah[i][e];
                        if (!(m == (_Float16)65504.f)) lof[i][e] = (_Float16)0.f;
                    }
#pragma unroll
                for (int i = 0; i < 4; ++i) bhf[i] = *reinterpret_cast<const h8 *>(b_lo + fb + i * 16 * RL_LD);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(lof[i], bhf[j], acc[i][j], 0, 0, 0);
            }
            if (tid == 0) s_sat[par ^ 1] = 0;       // read again two barriers from here, set again one barrier from here
        }
        __syncthreads();
    }

    // ---- epilogue: D[row 4 g + e][column l15] of each 16 x 16 tile; one lane reads and writes an element
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = c0 + wn * 64 + j * 16 + l15;
        if (col >= Nout) continue;
        const float b = bias ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = r0 + wm * 64 + i * 16 + g * 4 + e;
                if (row >= rows) continue;
                float v = acc[i][j][e] * inv_scale + b;
                if (act) v = gelu_tanh(v);
                if (residual) v = residual[(long long)row * ldr + col] + v;
                out[(long long)row * ldo + col] = v;
            }
    }
}

}  // namespace bt

namespace {

// do [a, a + na) and [b, b + nb) (bytes) share a byte
bool overlap(const void *a, unsigned long long na, const void *b, unsigned long long nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" int bt_rows_linear(const float *x, int64_t ldx, const void *w_hi, const void *w_lo, float inv_scale, const float *bias,
                              const float *residual, int64_t ldr, float *out, int64_t ldo,
                              int64_t rows, int64_t K, int64_t Nout, int prologue, float eps, int act, int precision, void *stream) {
    const int64_t MAXI = BT_ROWS_MAX_INDEX;
    if (!x || !w_hi || !w_lo || !out || rows < 0 || Nout < 1 || K < 8 || K % 8 != 0) return BT_EINVAL;
    if (ldx < K || ldo < Nout || (residual && ldr < Nout)) return BT_EINVAL;
    if ((prologue != BT_ROWS_PRO_NONE && prologue != BT_ROWS_PRO_LAYERNORM) || (act != BT_ROWS_ACT_NONE && act != BT_ROWS_ACT_GELU_TANH)
        || (precision != BT_ROWS_F16X3 && precision != BT_ROWS_F16))
        return BT_EINVAL;
    if (!std::isfinite(inv_scale) || !(inv_scale > 0.f)) return BT_EINVAL;
    if (prologue == BT_ROWS_PRO_LAYERNORM && (!std::isfinite(eps) || eps < 0.f)) return BT_EINVAL;
    if (rows > MAXI || K > MAXI || Nout > MAXI || ldx > MAXI || ldo > MAXI || (residual && ldr > MAXI)) return BT_EUNSUPPORTED;
    const int64_t n_rt = (rows + BT_ROWS_TILE - 1) / BT_ROWS_TILE, n_ct = (Nout + BT_ROWS_TILE - 1) / BT_ROWS_TILE;
    if (n_rt > 0 && n_ct > MAXI / n_rt) return BT_EUNSUPPORTED;
    if (rows == 0) return BT_OK;
    const unsigned long long x_bytes = ((unsigned long long)(rows - 1) * ldx + K) * 4, o_bytes = ((unsigned long long)(rows - 1) * ldo + Nout) * 4;
    if (overlap(out, o_bytes, x, x_bytes)) return BT_EINVAL;
    if (residual && !((const float *)out == residual && ldr == ldo)
        && overlap(out, o_bytes, residual, ((unsigned long long)(rows - 1) * ldr + Nout) * 4))
        return BT_EINVAL;
    const bool vec = (((uintptr_t)x | (uintptr_t)w_hi | (uintptr_t)w_lo) & 15) == 0 && ldx % 4 == 0;
    const bool x3 = precision == BT_ROWS_F16X3;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(n_rt * n_ct)), block(256);
    const unsigned short *wh = (const unsigned short *)w_hi, *wl = (const unsigned short *)w_lo;
#define BT_ROWS_LAUNCH(V, X)                                                                                                          \
    hipLaunchKernelGGL((bt::k_rows_linear<V, X>), grid, block, 0, st, x, (long long)ldx, wh, wl, inv_scale, bias, residual, (long long)ldr, \
                       out, (long long)ldo, (int)rows, (int)K, (int)Nout, (int)n_ct, prologue == BT_ROWS_PRO_LAYERNORM ? 1 : 0, eps,    \
                       act == BT_ROWS_ACT_GELU_TANH ? 1 : 0)
    if (vec && x3) BT_ROWS_LAUNCH(true, true);
    else if (vec) BT_ROWS_LAUNCH(true, false);
    else if (x3) BT_ROWS_LAUNCH(false, true);
    else BT_ROWS_LAUNCH(false, false);
#undef BT_ROWS_LAUNCH
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
