// attention.hip — fused float32 attention over strided sequences (include/batrack_attn.h holds the specification):
// k_attn_short (L <= 16, the transformers' time axis) and k_attn_long (the space axis).
//
// Both run on v_mfma_f32_16x16x4_f32 (D[i][j] += sum_k A[i][k] B[k][j]; lane l supplies A[l % 16][l / 16] and
// B[l / 16][l % 16] and holds D[4 (l / 16) + reg][l % 16]) and both compute the TRANSPOSED score tile, S^T = K . Q^T: a lane
// then holds one query (column l % 16) and the keys 4 g + reg (g = l / 16) of a tile of 16.  Hence
//   - the softmax of a query reduces over the lane's registers and over the four lanes l % 16 + 16 g;
//   - O^T = V^T . P^T takes register `reg` of S^T as it stands as the B operand of k-step `reg` (B[k = g] is key 4 g + reg);
//     the A operand of that step is V[key 4 g + reg][column 16 t + l % 16], the same permuted key order;
//   - O^T comes out with the query on the lane and four consecutive head columns in the registers: one float4 store;
//   - the contraction index of q . k is permuted the same way in both operands (k-step s, slice g is head column 12 g + s),
//     so that a lane loads its 12 columns of a row as three float4.
// k_attn_short: one wave per (sequence, head), operands straight from global memory.
// k_attn_long:  a workgroup of 4 waves per (sequence, head, tile of 128 queries), 2 query tiles of 16 per wave (two
//               independent accumulator chains, and every LDS fragment feeds two MFMAs); K and V in LDS tiles of 64 keys with
//               rows of 52 floats (the float4 reads of 16 key rows and the scalar reads of V hit 64 distinct banks), single
//               buffered: 26 KB a workgroup, so several workgroups share a CU and one stages while another multiplies.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/batrack_attn.h"
#include "../../include/batrack_ba.h"

namespace bt {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int AT_HD = BT_ATTN_HEAD_DIM, AT_THREADS = 256, AT_WAVES = AT_THREADS / 64;
constexpr int AT_KT = BT_ATTN_K_TILE, AT_QT = BT_ATTN_Q_TILE, AT_QW = AT_QT / AT_WAVES / 16;   // query tiles of 16 per wave
constexpr int AT_LD = AT_HD + 4, AT_C4 = AT_HD / 4;
static_assert(AT_HD == 48 && AT_KT == 64 && AT_QW == 2 && BT_ATTN_SHORT_L == 16, "the fragment maps below are written for these");

// 12 consecutive floats of a row (16-byte aligned when VEC)
template <bool VEC>
__device__ __forceinline__ void load12(const float *__restrict__ p, float *v) {
    if (VEC) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 t = *reinterpret_cast<const f32x4 *>(p + 4 * c);
            v[4 * c] = t[0]; v[4 * c + 1] = t[1]; v[4 * c + 2] = t[2]; v[4 * c + 3] = t[3];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 12; ++c) v[c] = p[c];
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float *__restrict__ p, f32x4 v) {
    if (VEC) *reinterpret_cast<f32x4 *>(p) = v;
    else { p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3]; }
}

__device__ __forceinline__ float group_sum(float v) {             // over the four lanes of a query: g ^ 1, then g ^ 2
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

__device__ __forceinline__ float group_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}

// ----------------------------------------------------------------------------------------------------------- k_attn_short
template <bool VEC>
__global__ __launch_bounds__(AT_THREADS) void k_attn_short(const float *__restrict__ qkv, long long qs, float *__restrict__ out,
                                                          long long os, int L, long long seq_stride, long long tok_stride, int heads,
                                                          float scale, long long nwork) {
#pragma clang fp contract(off)                                     // logit * scale - max as written: a fused form makes exp(0) inexact
    const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const long long w = (long long)blockIdx.x * AT_WAVES + (threadIdx.x >> 6);
    if (w >= nwork) return;                                        // (no barrier in this kernel)
    const int h = (int)(w % heads);
    const long long row0 = (w / heads) * seq_stride;
    const int hc = heads * AT_HD;
    const bool valid = l15 < L;                                    // this lane's query, and its key row of the first product

    float qf[12], kf[12];
#pragma unroll
    for (int s = 0; s < 12; ++s) qf[s] = kf[s] = 0.0f;
    if (valid) {
        const float *rp = qkv + (row0 + l15 * tok_stride) * qs + h * AT_HD + 12 * g;
        load12<VEC>(rp, qf);
        load12<VEC>(rp + hc, kf);
    }
    f32x4 sp[4];                                                   // four partial chains of 12 head columns: blocked, as a BLAS sums
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        sp[c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 3 * c; s < 3 * c + 3; ++s) sp[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s], qf[s], sp[c], 0, 0, 0);
    }
    f32x4 st = (sp[0] + sp[1]) + (sp[2] + sp[3]);                  // S^T: keys 4 g + r of query l15
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        st[r] = 4 * g + r < L ? st[r] * scale : -INFINITY;
        m = fmaxf(m, st[r]);
    }
    m = group_max(m);
    float den = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        st[r] = 4 * g + r < L ? expf(st[r] - m) : 0.0f;
        den += st[r];
    }
    den = group_sum(den);

    f32x4 o[2][3];                                                 // two chains: r even, r odd
#pragma unroll
    for (int t = 0; t < 3; ++t) o[0][t] = o[1][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = 4 * g + r;
        float va[3] = {0.0f, 0.0f, 0.0f};
        if (j < L) {
            const float *vp = qkv + (row0 + j * tok_stride) * qs + 2 * hc + h * AT_HD + l15;
#pragma unroll
            for (int t = 0; t < 3; ++t) va[t] = vp[16 * t];
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) o[r & 1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[t], st[r], o[r & 1][t], 0, 0, 0);
    }
    if (valid) {
        float *op = out + (row0 + l15 * tok_stride) * os + h * AT_HD + 4 * g;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const f32x4 n = o[0][t] + o[1][t];
            store4<VEC>(op + 16 * t, f32x4{n[0] / den, n[1] / den, n[2] / den, n[3] / den});
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ k_attn_long
template <bool VEC>
__global__ __launch_bounds__(AT_THREADS) void k_attn_long(const float *__restrict__ qkv, long long qs, float *__restrict__ out,
                                                         long long os, int L, long long seq_stride, long long tok_stride, int heads,
                                                         float scale, int qtiles) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float kl[AT_KT * AT_LD];
    __shared__ __attribute__((aligned(16))) float vl[AT_KT * AT_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    const long long bid = blockIdx.x;
    const int qt = (int)(bid % qtiles);
    const long long bh = bid / qtiles;
    const int h = (int)(bh % heads);
    const long long row0 = (bh / heads) * seq_stride;
    const int hc = heads * AT_HD;

    float qf[AT_QW][12];
    int qi[AT_QW];
#pragma unroll
    for (int c = 0; c < AT_QW; ++c) {
        qi[c] = qt * AT_QT + (wave * AT_QW + c) * 16 + l15;
#pragma unroll
        for (int s = 0; s < 12; ++s) qf[c][s] = 0.0f;
        if (qi[c] < L) load12<VEC>(qkv + (row0 + qi[c] * tok_stride) * qs + h * AT_HD + 12 * g, qf[c]);
    }
    f32x4 o[AT_QW][3];
    float m[AT_QW], den[AT_QW];
#pragma unroll
    for (int c = 0; c < AT_QW; ++c) {
        m[c] = -INFINITY;
        den[c] = 0.0f;
#pragma unroll
        for (int t = 0; t < 3; ++t) o[c][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    for (int k0 = 0; k0 < L; k0 += AT_KT) {
        __syncthreads();                                           // the previous tile has been read
        // ---- stage the tile: 64 keys x 12 float4, K then V; rows >= L are zeros and are never loaded
#pragma unroll
        for (int n = 0; n < 2 * AT_KT * AT_C4 / AT_THREADS; ++n) {
            const int idx = threadIdx.x + n * AT_THREADS;
            const int which = idx / (AT_KT * AT_C4), rem = idx - which * (AT_KT * AT_C4);
            const int key = rem / AT_C4, c4 = rem - key * AT_C4;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (k0 + key < L) {
                const float *p = qkv + (row0 + (k0 + key) * tok_stride) * qs + (1 + which) * hc + h * AT_HD + 4 * c4;
                if (VEC) v = *reinterpret_cast<const f32x4 *>(p);
                else v = f32x4{p[0], p[1], p[2], p[3]};
            }
            *reinterpret_cast<f32x4 *>((which ? vl : kl) + key * AT_LD + 4 * c4) = v;
        }
        __syncthreads();

        // ---- S^T = K . Q^T, four key tiles of 16
        f32x4 st[AT_QW][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float ka[12];
            load12<true>(kl + (16 * u + l15) * AT_LD + 12 * g, ka);
            f32x4 sp[AT_QW][2];                                    // two partial chains of 24 head columns (four cost a wave per SIMD in registers)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int c = 0; c < AT_QW; ++c) {
                    sp[c][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int s = 6 * n; s < 6 * n + 6; ++s) sp[c][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[s], qf[c][s], sp[c][n], 0, 0, 0);
                }
#pragma unroll
            for (int c = 0; c < AT_QW; ++c) st[c][u] = sp[c][0] + sp[c][1];
        }
        // ---- the online softmax of the two queries of this lane
#pragma unroll
        for (int c = 0; c < AT_QW; ++c) {
            float mx = -INFINITY;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    st[c][u][r] = k0 + 16 * u + 4 * g + r < L ? st[c][u][r] * scale : -INFINITY;
                    mx = fmaxf(mx, st[c][u][r]);
                }
            const float mn = fmaxf(m[c], group_max(mx));
            const float a = expf(m[c] - mn);
            m[c] = mn;
            float ps = 0.0f;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    st[c][u][r] = k0 + 16 * u + 4 * g + r < L ? expf(st[c][u][r] - mn) : 0.0f;
                    ps += st[c][u][r];
                }
            den[c] = den[c] * a + ps;
#pragma unroll
            for (int t = 0; t < 3; ++t) o[c][t] *= a;
        }
        // ---- O^T += V^T . P^T
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float *vp = vl + (16 * u + 4 * g + r) * AT_LD + l15;
                const float va[3] = {vp[0], vp[16], vp[32]};
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int c = 0; c < AT_QW; ++c) o[c][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[t], st[c][u][r], o[c][t], 0, 0, 0);
            }
    }
#pragma unroll
    for (int c = 0; c < AT_QW; ++c) {
        const float d = group_sum(den[c]);
        if (qi[c] < L) {
            float *op = out + (row0 + qi[c] * tok_stride) * os + h * AT_HD + 4 * g;
#pragma unroll
            for (int t = 0; t < 3; ++t)
                store4<VEC>(op + 16 * t, f32x4{o[c][t][0] / d, o[c][t][1] / d, o[c][t][2] / d, o[c][t][3] / d});
        }
    }
}

}  // namespace bt

extern "C" int bt_attention(const float *qkv, int64_t qkv_row_stride, float *out, int64_t out_row_stride,
                            int64_t n_seq, int64_t L, int64_t seq_stride, int64_t tok_stride,
                            int64_t heads, int64_t head_dim, float scale, void *stream) {
    const int64_t MAXI = BT_ATTN_MAX_INDEX;
    if (!qkv || !out || n_seq < 0 || L < 1 || heads < 1 || head_dim < 1 || seq_stride < 1 || tok_stride < 1 || !std::isfinite(scale))
        return BT_EINVAL;
    if (heads > INT64_MAX / 3 / head_dim) return BT_EINVAL;        // no row stride can hold that many columns
    if (qkv_row_stride < 3 * heads * head_dim || out_row_stride < heads * head_dim) return BT_EINVAL;
    if (head_dim != BT_ATTN_HEAD_DIM) return BT_EUNSUPPORTED;
    if (n_seq > MAXI || L > MAXI - BT_ATTN_Q_TILE || seq_stride > MAXI || tok_stride > MAXI || qkv_row_stride > MAXI || out_row_stride > MAXI)
        return BT_EUNSUPPORTED;
    if (n_seq == 0) return BT_OK;
    if ((n_seq - 1) * seq_stride + (L - 1) * tok_stride > MAXI) return BT_EUNSUPPORTED;       // each product is below 2^62
    const bool is_short = L <= BT_ATTN_SHORT_L;
    const int64_t qtiles = (L + BT_ATTN_Q_TILE - 1) / BT_ATTN_Q_TILE;
    if (n_seq > BT_ATTN_MAX_BLOCKS * 4 / heads || (!is_short && n_seq * heads > BT_ATTN_MAX_BLOCKS / qtiles)) return BT_EUNSUPPORTED;
    const int64_t blocks = is_short ? (n_seq * heads + bt::AT_WAVES - 1) / bt::AT_WAVES : n_seq * heads * qtiles;
    if (blocks > BT_ATTN_MAX_BLOCKS) return BT_EUNSUPPORTED;
    const bool vec = (((uintptr_t)qkv | (uintptr_t)out) & 15) == 0 && qkv_row_stride % 4 == 0 && out_row_stride % 4 == 0;
    const dim3 grid((unsigned)blocks), block(bt::AT_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (is_short) {
        const long long nwork = n_seq * heads;
        if (vec) hipLaunchKernelGGL(bt::k_attn_short<true>, grid, block, 0, st, qkv, (long long)qkv_row_stride, out, (long long)out_row_stride,
                                    (int)L, (long long)seq_stride, (long long)tok_stride, (int)heads, scale, nwork);
        else hipLaunchKernelGGL(bt::k_attn_short<false>, grid, block, 0, st, qkv, (long long)qkv_row_stride, out, (long long)out_row_stride,
                                (int)L, (long long)seq_stride, (long long)tok_stride, (int)heads, scale, nwork);
    } else {
        if (vec) hipLaunchKernelGGL(bt::k_attn_long<true>, grid, block, 0, st, qkv, (long long)qkv_row_stride, out, (long long)out_row_stride,
                                    (int)L, (long long)seq_stride, (long long)tok_stride, (int)heads, scale, (int)qtiles);
        else hipLaunchKernelGGL(bt::k_attn_long<false>, grid, block, 0, st, qkv, (long long)qkv_row_stride, out, (long long)out_row_stride,
                                (int)L, (long long)seq_stride, (long long)tok_stride, (int)heads, scale, (int)qtiles);
    }
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
