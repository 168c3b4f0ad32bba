// encoder_trunk.hip — one residual block of the feature encoder's layer1..4 (include/batrack_encoder.h holds the
// specification): k_res_conv, k_conv_stats (csrc/conv_stats.hip), k_res_join.
//
// k_res_conv<NORM, S, SHORT, NT> is a 3 x 3 convolution with zero padding 1 and stride S from c_in to 16 NT <= 128 channels, an
// implicit GEMM on v_mfma_f32_16x16x4_f32 with the tile of csrc/conv_tile.hpp (all 16 NT columns), K = 9 taps x c_in.
//   K-chunk  8 input channels at a time: their halo tile (18 x 10 input pixels at stride 1, 33 x 17 at stride 2, the even
//            columns of a row first) is staged in LDS beside their 9 x 8 x 16 NT weights.  NORM: a halo element inside the
//            input map is max(fl(fl(v - mean) * rstd), 0) with the (frame, channel)'s statistics, one outside is 0: the
//            padding is of the normalised, rectified map, which is never in memory.  Otherwise v, or 0 outside; the input is
//            a strided view.  At stride 1 the chunk's global loads go into registers while the chunk before it is multiplied
//            and reach LDS (normalised) when that one is done; at stride 2, with three accumulator sets, they are staged
//            directly, six unconditional loads at a time.  (The even/odd split is read from the code, not measured against
//            the interleaved row: it costs the staging one select.)
//   order    chunk ascending, tap, group of four channels; every CT_FLUSH = 2 chunks (144 products) the accumulators are
//            added into a second set and start again from zero; the bias last.  k_head_conv's order.
//   SHORT    the block's 1 x 1 stride-2 shortcut reads exactly the centre tap's staged pixel: a second GEMM from the same
//            chunk with the chunk's 8 x 16 NT shortcut weights, ONE fma chain over c_in products, the bias last, into a
//            second raw map with its own statistics.
//   output   raw = conv + bias as [F][16 NT][ho * wo] planes, and per (frame, tile, column) the float64 sum and sum of
//            squares of the stored values (tile_store_stats).
// k_conv_stats: one thread per (map, frame, channel) adds the tiles' partials in tile order and stores mean and rstd as floats.
// k_res_join: out = max(fl(s + max(fl(fl(raw2 - m2) * r2), 0)), 0); s = x (stride 1) or fl(fl(rawd - md) * rd) (stride 2).
// What they leave on the table is in DESIGN.md.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_encoder.h"
#include "conv_tile.hpp"

namespace bt {

constexpr int RC_MAXC = 128;

// -------------------------------------------------------------------------------------------------------------- k_res_conv
template <bool NORM, int S, bool SHORT, int NT>
__global__ __launch_bounds__(CT_THREADS) __attribute__((amdgpu_waves_per_eu(SHORT ? 1 : 2))) void k_res_conv(const ConvView X, int c_in, const float *__restrict__ mean, const float *__restrict__ rstd,
                                                         const float *__restrict__ wp, const float *__restrict__ bias,
                                                         const float *__restrict__ wd, const float *__restrict__ bd, int ho, int wo, int tiles_x,
                                                         float *__restrict__ raw, double *__restrict__ part, float *__restrict__ rawd,
                                                         double *__restrict__ partd) {
    using G = ConvGeom<S>;
    constexpr int COLS = 16 * NT, WLD = conv_wld(COLS), HW = G::HW, HALO = G::HALO, PL = G::PL;
    static_assert(9 * CT_KC * WLD * sizeof(float) >= (CT_THREADS / 64) * COLS * 2 * sizeof(double), "the statistics reuse the weights' LDS");
    static_assert(!SHORT || S == 2, "the shortcut belongs to the stride-2 block");
    __shared__ __attribute__((aligned(16))) float w_l[9 * CT_KC * WLD];          // [tap][channel of the chunk][WLD]
    __shared__ __attribute__((aligned(16))) float wd_l[SHORT ? CT_KC * WLD : 4];  // [channel of the chunk][WLD]
    __shared__ float in_l[CT_KC * PL];                                            // [channel of the chunk][halo pixel]
    __shared__ float mean_l[NORM ? RC_MAXC : 1], rstd_l[NORM ? RC_MAXC : 1];
    static_assert(sizeof(float) * (9 * CT_KC * WLD + (SHORT ? CT_KC * WLD : 4) + CT_KC * PL + (NORM ? 2 * RC_MAXC : 2)) <= 65536, "static LDS");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
    const int f = blockIdx.y, ty0 = (blockIdx.x / tiles_x) * CT_TH, tx0 = (blockIdx.x % tiles_x) * CT_TW;
    const int iy0 = S * ty0 - 1, ix0 = S * tx0 - 1;              // the halo's first input row and column
    const long long hwo = (long long)ho * wo;

    if constexpr (NORM) {
        for (int c = tid; c < c_in; c += CT_THREADS) { mean_l[c] = mean[(long long)f * c_in + c]; rstd_l[c] = rstd[(long long)f * c_in + c]; }
    }

    f32x4 acc[2][NT], tot[2][NT], accd[2][SHORT ? NT : 1];
    tile_zero<NT>(acc);
    tile_zero<NT>(tot);
    tile_zero<SHORT ? NT : 1>(accd);

    // Staging is split in two: the global loads of a chunk go into registers (`fetch`) while the chunk before it is
    // multiplied, and reach LDS (`stage`, which normalises) when that one is done.  The order of the sums does not change.
    constexpr int W4 = 9 * CT_KC * (COLS / 4), D4 = CT_KC * (COLS / 4), HE = CT_KC * HALO;
    constexpr int WN = (W4 + CT_THREADS - 1) / CT_THREADS, HN = (HE + CT_THREADS - 1) / CT_THREADS;
    static_assert(D4 <= CT_THREADS && HN <= 32, "one shortcut float4 a thread; the inside mask is 32 bits");
    f32x4 wreg[WN], dreg = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float hreg[HN];
    unsigned inside = 0;                                         // bit k: hreg[k] is an element of the input map
    const float *xf = X.p + (long long)f * X.sf;
    const int chunks = c_in / CT_KC;
    auto fetch = [&](int chunk) __attribute__((always_inline)) {
        const f32x4 *wsrc = reinterpret_cast<const f32x4 *>(wp + (size_t)chunk * 9 * CT_KC * COLS);
#pragma unroll
        for (int k = 0; k < WN; ++k) {
            const int i = tid + k * CT_THREADS;
            if (i < W4) wreg[k] = wsrc[i];
        }
        if constexpr (SHORT) {
            if (tid < D4) dreg = reinterpret_cast<const f32x4 *>(wd + (size_t)chunk * CT_KC * COLS)[tid];
        }
        const float *src = xf + (long long)chunk * CT_KC * X.sc;
        inside = 0;
#pragma unroll
        for (int k = 0; k < HN; ++k) {
            const int idx = tid + k * CT_THREADS;
            const int chl = idx / HALO, p = idx - chl * HALO, hy = p / HW, hx = p - hy * HW;
            const int gy = iy0 + hy, gx = ix0 + hx;
            float v = 0.0f;                                      // zero padding of the (normalised, rectified) input map
            if (idx < HE && gy >= 0 && gy < X.h && gx >= 0 && gx < X.w) {
                v = src[chl * X.sc + gy * X.sy + gx * X.sx];
                inside |= 1u << k;
            }
            hreg[k] = v;
        }
    };
    auto stage = [&](int chunk) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < WN; ++k) {
            const int i = tid + k * CT_THREADS;
            const int row = i / (COLS / 4), c4 = i - row * (COLS / 4);
            if (i < W4) *reinterpret_cast<f32x4 *>(w_l + row * WLD + c4 * 4) = wreg[k];
        }
        if constexpr (SHORT) {
            const int row = tid / (COLS / 4), c4 = tid - row * (COLS / 4);
            if (tid < D4) *reinterpret_cast<f32x4 *>(wd_l + row * WLD + c4 * 4) = dreg;
        }
#pragma unroll
        for (int k = 0; k < HN; ++k) {
            const int idx = tid + k * CT_THREADS;
            const int chl = idx / HALO, p = idx - chl * HALO, hy = p / HW, hx = p - hy * HW;
            float v = hreg[k];
            if constexpr (NORM) {
                if ((inside >> k) & 1u) {
                    const int c = chunk * CT_KC + chl;
                    v = norm_relu(v, mean_l[c], rstd_l[c]);
                }
            }
            const int col = S == 1 ? hx : ((hx & 1) ? G::EVEN + (hx >> 1) : (hx >> 1));
            if (idx < HE) in_l[chl * PL + hy * HW + col] = v;
        }
    };
    auto stage_direct = [&](int chunk) __attribute__((always_inline)) {      // the same elements to the same places, not through registers
        tile_stage_rows<9 * CT_KC, COLS, 3>(w_l, wp + (size_t)chunk * 9 * CT_KC * COLS, COLS);
        if constexpr (SHORT) tile_stage_rows<CT_KC, COLS>(wd_l, wd + (size_t)chunk * CT_KC * COLS, COLS);
        const float *src = xf + (long long)chunk * CT_KC * X.sc;
        // six loads at a time, every one unconditional (the address clamped into the map, the value dropped outside): a load
        // behind a branch that is used in its own trip waits for memory every trip
        constexpr int HB = 6;
#pragma unroll 1
        for (int k0 = 0; k0 < HN; k0 += HB) {
            float v[HB];
#pragma unroll
            for (int j = 0; j < HB; ++j) {
                const int idx = tid + (k0 + j) * CT_THREADS, ic = idx < HE ? idx : HE - 1;
                const int chl = ic / HALO, p = ic - chl * HALO, hy = p / HW, hx = p - hy * HW;
                const int gy = iy0 + hy, gx = ix0 + hx;
                const bool in = gy >= 0 && gy < X.h && gx >= 0 && gx < X.w;
                const int cy = gy < 0 ? 0 : (gy < X.h ? gy : X.h - 1), cx = gx < 0 ? 0 : (gx < X.w ? gx : X.w - 1);
                float t = src[chl * X.sc + cy * X.sy + cx * X.sx];
                if constexpr (NORM) {
                    const int c = chunk * CT_KC + chl;
                    t = norm_relu(t, mean_l[c], rstd_l[c]);
                }
                v[j] = in ? t : 0.0f;                            // zero padding of the (normalised, rectified) input map
            }
#pragma unroll
            for (int j = 0; j < HB; ++j) {
                const int idx = tid + (k0 + j) * CT_THREADS;
                const int chl = idx / HALO, p = idx - chl * HALO, hy = p / HW, hx = p - hy * HW;
                const int col = S == 1 ? hx : ((hx & 1) ? G::EVEN + (hx >> 1) : (hx >> 1));
                if (idx < HE) in_l[chl * PL + hy * HW + col] = v[j];
            }
        }
    };
    // stride 2 stages directly: 18 halo registers on top of its three accumulator sets spill (kernel-resource-usage), and it
    // is a twelfth of the trunk's products
    constexpr bool AHEAD = S == 1;
    if constexpr (AHEAD) fetch(0);
    for (int chunk = 0; chunk < chunks; ++chunk) {
        __syncthreads();                                         // the previous chunk's reads are done (and the statistics are written)
        if constexpr (AHEAD) stage(chunk);
        else stage_direct(chunk);
        __syncthreads();
        if constexpr (AHEAD) {
            if (chunk + 1 < chunks) fetch(chunk + 1);            // in flight while this chunk is multiplied
        }
        if constexpr (SHORT)                                     // the centre tap's pixel is the shortcut's
            tile_taps<S, NT>(in_l, w_l, acc, [&](int s, float a0, float a1) __attribute__((always_inline)) { tile_group<NT>(a0, a1, wd_l + (4 * s + q) * WLD + l16, accd); });
        else
            tile_taps<S, NT>(in_l, w_l, acc);
        if (chunk % CT_FLUSH == CT_FLUSH - 1) tile_flush<NT>(tot, acc);      // a block is complete: one rounded add into the total
    }
    __syncthreads();                                             // the last chunk's weights are read: their LDS takes the statistics
    double *red = reinterpret_cast<double *>(w_l);
    const long long tile = (long long)f * gridDim.x + blockIdx.x;
    tile_store_stats<NT, true>(tot, bias, raw + (long long)f * COLS * hwo, hwo, ho, wo, ty0, tx0, red, part + tile * COLS * 2);
    if constexpr (SHORT) {
        __syncthreads();                                         // `red` is read
        tile_store_stats<NT, true>(accd, bd, rawd + (long long)f * COLS * hwo, hwo, ho, wo, ty0, tx0, red, partd + tile * COLS * 2);
    }
}

// -------------------------------------------------------------------------------------------------------------- k_res_join
// raw2, rawd [F][C][n]; the statistics [F][C]; X the block's input (DOWN: unused); out [F][C][n].  V pixels a thread.
template <bool DOWN, int V>
__global__ __launch_bounds__(256) void k_res_join(const float *__restrict__ raw2, const float *__restrict__ m2, const float *__restrict__ r2,
                                                  const float *__restrict__ rawd, const float *__restrict__ md, const float *__restrict__ rd,
                                                  const ConvView X, int C, int wo, long long n, float *__restrict__ out) {
    const int c = blockIdx.y, f = blockIdx.z;
    const long long p = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (p >= n) return;
    const long long fc = (long long)f * C + c, base = fc * n + p;
    const float mean2 = m2[fc], rstd2 = r2[fc];
    float y[V], s[V];
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(raw2 + base);
        y[0] = t.x; y[1] = t.y; y[2] = t.z; y[3] = t.w;
    } else {
        y[0] = raw2[base];
    }
    if (DOWN) {
        const float meand = md[fc], rstdd = rd[fc];
        if constexpr (V == 4) {
            const float4 t = *reinterpret_cast<const float4 *>(rawd + base);
            s[0] = t.x; s[1] = t.y; s[2] = t.z; s[3] = t.w;
        } else {
            s[0] = rawd[base];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) s[j] = norm_plain(s[j], meand, rstdd);
    } else {
        const int py = (int)(p / wo), px = (int)(p - (long long)py * wo);
        const float *xs = X.p + f * X.sf + c * X.sc + py * X.sy + px * X.sx;
        if constexpr (V == 4) {                                            // V == 4 only with unit x stride, wo % 4 == 0 and 16-byte rows
            const float4 t = *reinterpret_cast<const float4 *>(xs);
            s[0] = t.x; s[1] = t.y; s[2] = t.z; s[3] = t.w;
        } else {
            s[0] = xs[0];
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float z = __fadd_rn(s[j], norm_relu(y[j], mean2, rstd2));
        y[j] = z > 0.0f ? z : 0.0f;
    }
    if constexpr (V == 4) *reinterpret_cast<float4 *>(out + base) = float4{y[0], y[1], y[2], y[3]};
    else out[base] = y[0];
}

static bool res_channels(long long c) { return c == 64 || c == 96 || c == 128; }

// maps = 2 (raw1, raw2) or 3 (raw1, rawd, raw2) raw maps, sets of partials and sets of statistics; false when the sizes are refused
static bool res_layout(long long F, long long c_out, long long h, long long w, long long stride, ConvLayout *L) {
    if (!res_channels(c_out) || (stride != 1 && stride != 2)) return false;
    const int maps = stride == 1 ? 2 : 3;
    return conv_layout(F, c_out, conv_out(h, stride), conv_out(w, stride), maps, maps, maps, L);
}

template <bool NORM, int S, bool SHORT>
static bool res_conv_launch(hipStream_t st, long long tiles, long long F, long long c_out, const ConvView &X, int c_in, const float *mean, const float *rstd,
                            const float *wp, const float *bias, const float *wd, const float *bd, int ho, int wo, int tiles_x, float *raw, double *part,
                            float *rawd, double *partd) {
    const dim3 grid((unsigned)tiles, (unsigned)F), block(CT_THREADS);
    if (c_out == 64)
        hipLaunchKernelGGL((k_res_conv<NORM, S, SHORT, 4>), grid, block, 0, st, X, c_in, mean, rstd, wp, bias, wd, bd, ho, wo, tiles_x, raw, part, rawd, partd);
    else if (c_out == 96)
        hipLaunchKernelGGL((k_res_conv<NORM, S, SHORT, 6>), grid, block, 0, st, X, c_in, mean, rstd, wp, bias, wd, bd, ho, wo, tiles_x, raw, part, rawd, partd);
    else
        hipLaunchKernelGGL((k_res_conv<NORM, S, SHORT, 8>), grid, block, 0, st, X, c_in, mean, rstd, wp, bias, wd, bd, ho, wo, tiles_x, raw, part, rawd, partd);
    return hipGetLastError() == hipSuccess;
}

}  // namespace bt

extern "C" size_t bt_res_block_workspace_bytes(int64_t F, int64_t c_out, int64_t h_in, int64_t w_in, int64_t stride) {
    bt::ConvLayout L;
    return bt::res_layout(F, c_out, h_in, w_in, stride, &L) ? L.bytes : 0;
}

extern "C" int bt_res_block(const bt_encoder_level *x, const struct bt_res_block *blk, int64_t F, void *workspace, float *out, void *stream) {
    using namespace bt;
    if (level_invalid(x) || !blk || !workspace || !out || !blk->w1 || !blk->b1 || !blk->w2 || !blk->b2) return BT_EINVAL;
    if (F < 1 || x->C < 1 || blk->c_in < 1 || blk->c_out < 1 || blk->stride < 1) return BT_EINVAL;
    if (((uintptr_t)blk->w1 & 15) || ((uintptr_t)blk->w2 & 15) || ((uintptr_t)blk->wd & 15) || ((uintptr_t)workspace & 15)) return BT_EINVAL;
    if (blk->stride == 1 && (blk->wd || blk->bd)) return BT_EINVAL;
    if (blk->stride == 2 && (!blk->wd || !blk->bd)) return BT_EINVAL;
    const long long c_in = blk->c_in, c_out = blk->c_out, stride = blk->stride;
    if (!res_channels(c_in) || !res_channels(c_out) || stride > 2 || (stride == 1 && c_in != c_out) || F > 65535) return BT_EUNSUPPORTED;
    if (level_check(x, c_in, F) != BT_OK) return BT_EUNSUPPORTED;
    ConvLayout L;
    if (!res_layout(F, c_out, x->h, x->w, stride, &L)) return BT_EUNSUPPORTED;

    // slot 0 is raw1's, the last raw2's, and at stride 2 the shortcut's lies between them: raw1's statistics and the
    // shortcut's are one launch
    hipStream_t st = (hipStream_t)stream;
    const bool down = stride == 2;
    const long long last = down ? 2 : 1;
    float *raw1 = (float *)workspace, *rawd = down ? raw1 + L.raw_slot : nullptr, *raw2 = raw1 + last * L.raw_slot;
    double *part1 = (double *)((char *)workspace + L.part), *partd = down ? part1 + L.part_slot : nullptr, *part2 = part1 + last * L.part_slot;
    float *mean1 = (float *)((char *)workspace + L.stat), *rstd1 = mean1 + (last + 1) * L.stat_slot;
    float *meand = down ? mean1 + L.stat_slot : nullptr, *rstdd = down ? rstd1 + L.stat_slot : nullptr;
    float *mean2 = mean1 + last * L.stat_slot, *rstd2 = rstd1 + last * L.stat_slot;
    const int ho = (int)conv_out(x->h, stride), wo = (int)conv_out(x->w, stride), tiles_x = (int)conv_tiles_x(wo);
    const ConvView X = conv_view(*x), Y{raw1, c_out * L.n, L.n, wo, 1, ho, wo};

    bool ok = down
        ? res_conv_launch<false, 2, true>(st, L.tiles, F, c_out, X, (int)c_in, nullptr, nullptr, blk->w1, blk->b1, blk->wd, blk->bd, ho, wo, tiles_x, raw1, part1, rawd, partd)
        : res_conv_launch<false, 1, false>(st, L.tiles, F, c_out, X, (int)c_in, nullptr, nullptr, blk->w1, blk->b1, nullptr, nullptr, ho, wo, tiles_x, raw1, part1, nullptr, nullptr);
    if (!ok || !conv_stats_launch(st, part1, L.tiles, c_out, last * L.stat_slot, L.n, mean1, rstd1)) return BT_EHIP;
    if (!res_conv_launch<true, 1, false>(st, L.tiles, F, c_out, Y, (int)c_out, mean1, rstd1, blk->w2, blk->b2, nullptr, nullptr, ho, wo, tiles_x, raw2, part2,
                                         nullptr, nullptr)
        || !conv_stats_launch(st, part2, L.tiles, c_out, L.stat_slot, L.n, mean2, rstd2))
        return BT_EHIP;

    // four pixels a thread: 16-byte rows of out and of the raw maps, and at stride 1 of x too
    const bool rows16 = L.n % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const bool xrows16 = rows16 && wo % 4 == 0 && x->sx == 1 && x->sy % 4 == 0 && x->sc % 4 == 0 && x->sf % 4 == 0 && ((uintptr_t)x->data & 15) == 0;
    ok = pointwise_launch(down ? k_res_join<true, 4> : k_res_join<false, 4>, down ? k_res_join<true, 1> : k_res_join<false, 1>, down ? rows16 : xrows16,
                          L.n, c_out, F, st, raw2, mean2, rstd2, rawd, meand, rstdd, X, (int)c_out, wo, L.n, out);
    return ok ? BT_OK : BT_EHIP;
}
