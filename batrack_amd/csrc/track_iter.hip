// track_iter.hip — the tracker's refinement iteration around its update transformers (include/batrack_track.h holds the
// specification): k_pos_embed, k_track_tokens, k_track_apply.
//
// k_track_tokens and k_track_apply carry a small matrix product each ([tokens x 195] . [195 x F] and [tokens x C] . [C x C]).
// Both run it on the matrix cores, one 16-token tile per wave at a time: the A operand is COMPUTED in the lane that owns it
// (lane l holds row l % 16, k-slice l / 16), the weight fragments come from LDS, transposed once per block.  The tokens'
// product is v_mfma_f32_16x16x4_f32 (its inputs carry the rounding of a float32 argument of up to 1e5 rad: a float32 fma
// chain adds nothing that shows).  The state update's is v_mfma_f64_16x16x4_f64 with the row normalised in double: the
// products of float32 values are exact there, so each feature carries the rounding of erff and of its last add only.  (A
// 128-term float32 fma chain was built first: on the fixture's one-token case it was 4.2e-7 from the reference's float32
// run, whose own distance to its float64 run is 1.7e-7 there — the chain rounds more than the reference's blocked sum.)
//   tokens: the 195 inputs are taken in the kernel's own order so that no lane evaluates a sine it does not use: k-slice q
//           owns the 24 (axis, frequency) pairs 24q .. 24q+23 and feeds sin then cos of each over steps 0 .. 47; step 48
//           carries the flow itself in slices 0 .. 2 (slice 3 is the zero padding of K to 196).  LDS: 196 rows of 145 floats.
//   apply:  the wave's 16 rows of delta are one contiguous block of 16 (3 + C) floats: copied to LDS coalesced, normalised
//           on the way into the A operand (k = 4 step + q, the natural order).  LDS: C rows of C + 17 floats and the tiles.
// Row strides are odd so that the transposing fill writes without bank conflicts; the fragment reads then meet one two-way
// conflict per half wave.
// A VALU form with LDS-broadcast weights was not built: the MFMA form needs one VGPR per operand and leaves the VALU to
// sincosf, which is the other half of the token kernel's work.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_track.h"
#include "dev_cache.hpp"
#include "sample_taps.hpp"

namespace bt {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int TI_PE_THREADS = 256;

constexpr int TK_THREADS = 512, TK_WAVES = TK_THREADS / 64;
constexpr int TK_K = 196, TK_NT = BT_TRACK_MAX_F / 16, TK_LD = BT_TRACK_MAX_F + 1;      // 196 x 145 floats = 113680 B
constexpr size_t TK_LDS = (size_t)TK_K * TK_LD * sizeof(float);

constexpr int AP_THREADS = 256, AP_WAVES = AP_THREADS / 64, AP_NT = BT_TRACK_MAX_C / 16;

#define BT_TI_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// ------------------------------------------------------------------------------------------------------------ k_pos_embed
// one thread per (point, column); model_utils.py:94-154 on the separable table
__global__ __launch_bounds__(TI_PE_THREADS) void k_pos_embed(const float *__restrict__ tabx, const float *__restrict__ taby, int H, int W,
                                                            int E, const float *__restrict__ coords, long long cstride, long long total,
                                                            float *__restrict__ out) {
#pragma clang fp contract(off)
    const int E2 = E / 2;
    for (long long i = (long long)blockIdx.x * TI_PE_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * TI_PE_THREADS) {
        const long long n = i / E;
        const int col = (int)(i - n * E);
        const float x = coords[n * cstride], y = coords[n * cstride + 1];
        const int x0 = floor_int(x), y0 = floor_int(y);
        const long long x1 = (long long)x0 + 1, y1 = (long long)y0 + 1;
        const float x0f = (float)x0, x1f = (float)x1, y0f = (float)y0, y1f = (float)y1;
        const long long mx = W - 1, my = H - 1;
        const long long cx0 = x0 < 0 ? 0 : (x0 > mx ? mx : x0), cx1 = x1 < 0 ? 0 : (x1 > mx ? mx : x1);
        const long long cy0 = y0 < 0 ? 0 : (y0 > my ? my : y0), cy1 = y1 < 0 ? 0 : (y1 > my ? my : y1);
        float i00, i01, i10, i11;
        if (col < E2) {
            i00 = i10 = tabx[cx0 * E2 + col];
            i01 = i11 = tabx[cx1 * E2 + col];
        } else {
            i00 = i01 = taby[cy0 * E2 + (col - E2)];
            i10 = i11 = taby[cy1 * E2 + (col - E2)];
        }
        const float w00 = (x1f - x) * (y1f - y), w01 = (x - x0f) * (y1f - y), w10 = (x1f - x) * (y - y0f), w11 = (x - x0f) * (y - y0f);
        out[i] = ((w00 * i00 + w01 * i01) + w10 * i10) + w11 * i11;
    }
}

// --------------------------------------------------------------------------------------------------------- k_track_tokens
// which of the 195 embedding inputs LDS row r = 4 step + q holds (-1: the padding)
__device__ __forceinline__ int tk_input_of_row(int r) {
    const int step = r >> 2, q = r & 3;
    if (step == 48) return q < 3 ? 192 + q : -1;
    const int p = q * 24 + (step >> 1);                          // (axis, frequency) pair: axis p / 32, frequency p % 32
    return (p >> 5) * 64 + 2 * (p & 31) + (step & 1);
}

__global__ __launch_bounds__(TK_THREADS) void k_track_tokens(const float *__restrict__ coords, const float *__restrict__ coords_sub,
                                                            const float *__restrict__ fcorrs, const float *__restrict__ ffeats,
                                                            const float *__restrict__ track_mask, const float *__restrict__ vis,
                                                            const float *__restrict__ pos, const float *__restrict__ time,
                                                            const float *__restrict__ w_flow, const float *__restrict__ b_flow,
                                                            int S, long long N, int F, int LRR, int C, int fix_track_mask,
                                                            float *__restrict__ x, long long tokens, long long ntiles) {
    extern __shared__ __attribute__((aligned(16))) float wl[];   // [TK_K][TK_LD]: wl[r][col] = W_flow[col][input of row r]
    for (int idx = threadIdx.x; idx < TK_K * BT_TRACK_MAX_F; idx += TK_THREADS) {
        const int col = idx / TK_K, r = idx - col * TK_K;
        const int k = tk_input_of_row(r);
        wl[r * TK_LD + col] = (col < F && k >= 0) ? w_flow[(long long)col * BT_TRACK_EMB + k] : 0.0f;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l16 = lane & 15, q = lane >> 4;
    const int E = F + LRR + C + 2;
    for (long long tile = (long long)blockIdx.x * TK_WAVES + wave; tile < ntiles; tile += (long long)gridDim.x * TK_WAVES) {
        // ---- the flow of this lane's row
        const long long tok = tile * 16 + l16;
        const bool valid = tok < tokens;
        float fl[3] = {0.0f, 0.0f, 0.0f};
        if (valid) {
            const long long n = tok / S;
            const int t = (int)(tok - n * S);
            const long long at = ((long long)t * N + n) * 3, a0 = n * 3;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                float ct = coords[at + d], c0 = coords[a0 + d];
                if (coords_sub) { ct = __fsub_rn(ct, coords_sub[at + d]); c0 = __fsub_rn(c0, coords_sub[a0 + d]); }
                fl[d] = __fsub_rn(ct, c0);
            }
        }
        f32x4 acc[TK_NT];
#pragma unroll
        for (int ct = 0; ct < TK_NT; ++ct) acc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const float *wq = wl + q * TK_LD + l16;
#pragma unroll 2
        for (int i = 0; i < 24; ++i) {
            const int p = q * 24 + i, axis = p >> 5;
            const float v = axis == 0 ? fl[0] : (axis == 1 ? fl[1] : fl[2]);
            const float arg = __fmul_rn(v, (float)(2 * (p & 31)) * 15.625f);
            float sn, cs;
            sincosf(arg, &sn, &cs);
            if (!valid) { sn = 0.0f; cs = 0.0f; }
            const float *w0 = wq + (8 * i) * TK_LD, *w1 = w0 + 4 * TK_LD;
#pragma unroll
            for (int ct = 0; ct < TK_NT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(sn, w0[ct * 16], acc[ct], 0, 0, 0);
#pragma unroll
            for (int ct = 0; ct < TK_NT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(cs, w1[ct * 16], acc[ct], 0, 0, 0);
        }
        {
            const float a = q == 0 ? fl[0] : (q == 1 ? fl[1] : (q == 2 ? fl[2] : 0.0f));
            const float *w0 = wq + (4 * 48) * TK_LD;
#pragma unroll
            for (int ct = 0; ct < TK_NT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w0[ct * 16], acc[ct], 0, 0, 0);
        }
        // ---- the flow columns: register j of lane l is row 4 (l / 16) + j, column 16 ct + l % 16
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long tr = tile * 16 + 4 * q + j;
            if (tr < tokens) {
                const long long n = tr / S;
                const int t = (int)(tr - n * S);
                float *xr = x + tr * E;
                const float *pr = pos + n * E, *tm = time + (long long)t * E;
#pragma unroll
                for (int ct = 0; ct < TK_NT; ++ct) {
                    const int col = ct * 16 + l16;
                    if (col < F) xr[col] = __fadd_rn(__fadd_rn(__fadd_rn(acc[ct][j], b_flow[col]), pr[col]), tm[col]);
                }
            }
        }
        // ---- the copy columns, a row at a time, the wave across the columns
        const int ncopy = LRR + C + 2;
        for (int r = 0; r < 16; ++r) {
            const long long tr = tile * 16 + r;
            if (tr >= tokens) break;
            const long long n = tr / S;
            const int t = (int)(tr - n * S);
            const long long sn = (long long)t * N + n;
            float *xr = x + tr * E + F;
            const float *pr = pos + n * E + F, *tm = time + (long long)t * E + F;
            for (int c = lane; c < ncopy; c += 64) {
                float v;
                if (c < LRR) v = fcorrs[sn * LRR + c];
                else if (c < LRR + C) v = ffeats[sn * C + (c - LRR)];
                else {
                    const int slot = c - LRR - C;
                    if (fix_track_mask) v = slot == 0 ? track_mask[sn] : vis[sn];
                    else {
                        const long long f = n * 2 * S + 2 * t + slot, m = f / S;
                        const long long s = f - m * S;
                        v = m < N ? track_mask[s * N + m] : vis[s * N + (m - N)];
                    }
                }
                xr[c] = __fadd_rn(__fadd_rn(v, pr[c]), tm[c]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- k_track_apply
__global__ __launch_bounds__(AP_THREADS) void k_track_apply(const float *__restrict__ delta, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, const float *__restrict__ w_u,
                                                           const float *__restrict__ b_u, float *__restrict__ state,
                                                           float *__restrict__ ffeats, const float *__restrict__ total,
                                                           const float *__restrict__ dyn_mask, int S, long long N, int C,
                                                           float stride, float Dz, float d_range, float d_near, int use_log_depth,
                                                           float *__restrict__ out, long long tokens, long long ntiles) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = C + 17, D = C + 3;
    float *wl = lds;                                              // [C][LD]: wl[k][col] = W_u[col][k]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *st = lds + C * LD + wave * 16 * D;                     // this wave's 16 rows of delta
    for (int idx = threadIdx.x; idx < C * C; idx += AP_THREADS) {
        const int col = idx / C, k = idx - col * C;
        wl[k * LD + col] = w_u[idx];
    }
    __syncthreads();

    const int l16 = lane & 15, q = lane >> 4, nt = C / 16, ksteps = C / 4;
    const double inv_c = 1.0 / (double)C;
    for (long long tile = (long long)blockIdx.x * AP_WAVES + wave; tile < ntiles; tile += (long long)gridDim.x * AP_WAVES) {
        const long long tok0 = tile * 16;
        const int rows = tokens - tok0 < 16 ? (int)(tokens - tok0) : 16;
        BT_TI_WAVE_SYNC();                                       // the previous tile's reads are done
        for (int i = lane; i < rows * D; i += 64) st[i] = delta[tok0 * D + i];
        BT_TI_WAVE_SYNC();
        // ---- coordinates: lanes 0 .. 47 are (row, component)
        if (lane < rows * 3) {
            const int r = lane / 3, d = lane - 3 * r;
            const long long tr = tok0 + r, n = tr / S;
            const int t = (int)(tr - n * S);
            const long long at = ((long long)t * N + n) * 3 + d;
            const float c = __fadd_rn(state[at], st[r * D + d]);
            state[at] = c;
            float p = c;
            if (total) p = __fsub_rn(total[at], __fmul_rn(c, dyn_mask[n]));
            float o;
            if (d < 2) o = __fmul_rn(p, stride);
            else {
                o = __fadd_rn(__fmul_rn(__fdiv_rn(p, Dz), d_range), d_near);
                if (use_log_depth) o = expf(o);
            }
            out[at] = o;
        }
        // ---- the row's moments: this lane holds channels 4 j + q of row l16
        const bool valid = l16 < rows;
        const float *row = st + l16 * D + 3 + q;
        double sum = 0.0;
        if (valid) for (int j = 0; j < ksteps; ++j) sum += (double)row[4 * j];
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const double mean = sum * inv_c;
        double ss = 0.0;
        if (valid) for (int j = 0; j < ksteps; ++j) { const double dv = (double)row[4 * j] - mean; ss += dv * dv; }
        ss += __shfl_xor(ss, 16);
        ss += __shfl_xor(ss, 32);
        const double rstd = 1.0 / sqrt(ss * inv_c + 1e-5);
        f64x4 acc[AP_NT];
#pragma unroll
        for (int ct = 0; ct < AP_NT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
        const float *wq = wl + q * LD + l16;
        for (int j = 0; j < ksteps; ++j) {
            const int k = 4 * j + q;
            const double a = valid ? ((double)row[4 * j] - mean) * rstd * (double)gamma[k] + (double)beta[k] : 0.0;
            const float *w0 = wq + 4 * j * LD;
#pragma unroll
            for (int ct = 0; ct < AP_NT; ++ct)
                if (ct < nt) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)w0[ct * 16], acc[ct], 0, 0, 0);
        }
        // register j of lane l is row (l / 16) + 4 j, column 16 ct + l % 16 (the f64 result layout, not the f32 one)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = q + 4 * j;
            if (r < rows) {
                const long long tr = tok0 + r, n = tr / S;
                const int t = (int)(tr - n * S);
                float *fr = ffeats + ((long long)t * N + n) * C;
#pragma unroll
                for (int ct = 0; ct < AP_NT; ++ct)
                    if (ct < nt) {
                        const int col = ct * 16 + l16;
                        const float v = (float)(acc[ct][j] + (double)b_u[col]);
                        fr[col] += 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
                    }
            }
        }
    }
}

static bool tiles_grid(long long ntiles, int waves, unsigned *grid) {
    DevProps dp;
    if (!device_props(&dp)) return false;
    const long long blocks = (ntiles + waves - 1) / waves;
    *grid = (unsigned)(blocks < dp.n_cu ? blocks : dp.n_cu);   // one block a CU: the weight fragments take most of its LDS
    return true;
}

}  // namespace bt

extern "C" int bt_track_pos_embed(const float *tabx, const float *taby, int64_t H, int64_t W, int64_t E,
                                  const float *coords, int64_t coord_stride, int64_t N, float *out, void *stream) {
    if (!tabx || !taby || !coords || !out || H < 1 || W < 1 || E < 2 || (E & 1) || coord_stride < 2 || N < 0) return BT_EINVAL;
    if (H > 32768 || W > 32768 || E > 65536 || N > 2147483647LL - 16) return BT_EUNSUPPORTED;
    if (N == 0) return BT_OK;
    const long long total = (long long)N * E;
    const long long nb = (total + bt::TI_PE_THREADS - 1) / bt::TI_PE_THREADS;
    hipLaunchKernelGGL(bt::k_pos_embed, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(bt::TI_PE_THREADS), 0, (hipStream_t)stream,
                       tabx, taby, (int)H, (int)W, (int)E, coords, (long long)coord_stride, total, out);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

extern "C" int bt_track_tokens(const float *coords, const float *coords_sub, const float *fcorrs, const float *ffeats,
                               const float *track_mask, const float *vis, const float *pos, const float *time,
                               const float *w_flow, const float *b_flow, int64_t S, int64_t N, int64_t F, int64_t LRR, int64_t C,
                               int32_t fix_track_mask, float *x, void *stream) {
    if (!coords || !fcorrs || !ffeats || !track_mask || !vis || !pos || !time || !w_flow || !b_flow || !x) return BT_EINVAL;
    if (S < 1 || N < 0 || F < 1 || LRR < 1 || C < 1) return BT_EINVAL;
    if (F > BT_TRACK_MAX_F || LRR > 65536 || C > 65536 || S > 2147483647LL - 16 || N > 2147483647LL - 16 || S * N > 2147483647LL - 16)
        return BT_EUNSUPPORTED;
    if (N == 0) return BT_OK;
    const long long tokens = (long long)S * N, ntiles = (tokens + 15) / 16;
    unsigned grid;
    static bt::LdsLimit lds_limit;
    if (!bt::tiles_grid(ntiles, bt::TK_WAVES, &grid) || !lds_limit.ensure((const void *)bt::k_track_tokens, bt::TK_LDS)) return BT_EHIP;
    hipLaunchKernelGGL(bt::k_track_tokens, dim3(grid), dim3(bt::TK_THREADS), bt::TK_LDS, (hipStream_t)stream, coords, coords_sub, fcorrs,
                       ffeats, track_mask, vis, pos, time, w_flow, b_flow, (int)S, (long long)N, (int)F, (int)LRR, (int)C,
                       (int)fix_track_mask, x, tokens, ntiles);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

extern "C" int bt_track_apply(const float *delta, const float *gamma, const float *beta, const float *w_u, const float *b_u,
                              float *state, float *ffeats, const float *total, const float *dyn_mask,
                              int64_t S, int64_t N, int64_t C, float stride, float Dz, float d_range, float d_near,
                              int32_t use_log_depth, float *out, void *stream) {
    if (!delta || !gamma || !beta || !w_u || !b_u || !state || !ffeats || !out || (total && !dyn_mask)) return BT_EINVAL;
    if (S < 1 || N < 0 || C < 1 || (C & 15)) return BT_EINVAL;
    if (C > BT_TRACK_MAX_C || S > 2147483647LL - 16 || N > 2147483647LL - 16 || S * N > 2147483647LL - 16) return BT_EUNSUPPORTED;
    if (N == 0) return BT_OK;
    const long long tokens = (long long)S * N, ntiles = (tokens + 15) / 16;
    const size_t lds = ((size_t)C * (C + 17) + (size_t)bt::AP_WAVES * 16 * (C + 3)) * sizeof(float);
    unsigned grid;
    static bt::LdsLimit lds_limit;
    if (!bt::tiles_grid(ntiles, bt::AP_WAVES, &grid) || !lds_limit.ensure((const void *)bt::k_track_apply, lds)) return BT_EHIP;
    hipLaunchKernelGGL(bt::k_track_apply, dim3(grid), dim3(bt::AP_THREADS), lds, (hipStream_t)stream, delta, gamma, beta, w_u, b_u,
                       state, ffeats, total, dyn_mask, (int)S, (long long)N, (int)C, stride, Dz, d_range, d_near, (int)use_log_depth,
                       out, tokens, ntiles);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
