// encoder_stem.hip — the feature encoder's stem, conv1 7 x 7 stride 2 from 3 to 64 channels, norm1, relu1
// (include/batrack_encoder.h holds the specification): k_stem_conv, k_conv_stats (csrc/conv_stats.hip), k_stem_norm.
//
// k_stem_conv is an implicit GEMM on v_mfma_f32_16x16x4_f32 with the tile of csrc/conv_tile.hpp (16 x 8 output pixels, four
// waves, all 64 columns: NT = 4).  K = (ky, c, kx) with kx padded from 7 to 8 by a zero weight: 168 rows, 42 groups of four.
//   weights  the whole packed weight, [168][64], is resident in LDS as rows of conv_wld(64) floats (53760 bytes), staged
//            once for the ST_TPW = 3 tiles a workgroup takes one after the other; a tile's halo is loaded into registers
//            while the tile before it is multiplied.
//   halo     37 x 21 input pixels x 3 channels, staged as 38 columns: column 37 meets only the zero weight and is written as
//            0 (a defined operand: NaN x 0 is NaN), as is every pixel outside the image (the zero padding of the IMAGE).  The
//            even columns of all rows come first, [c][row][19], the odd ones after them from ST_ODD on, which is 16 mod 32:
//            lane l / 16 of a group reads kx = 4 g + l / 16, so the two 16-lane rows of a 32-lane half read an even and an
//            odd part, at unit lane stride each and on different banks.
//   order    ky ascending, then c, then the two groups of four kx (the MFMA is a float32 fma chain, kx ascending); after
//            every ky (21 products and 3 zeros) the chain is added into the total and starts again; the bias last.
//   output   raw = conv + bias straight into out's [F][64][ho * wo] planes, a lane's four pixels as one float4 where the rows
//            allow, and per (frame, tile, column) the float64 sum and sum of squares of the stored values (tile_store_stats).
// k_conv_stats: one thread per (frame, channel) adds the tiles' partials in tile order (tile_order_stats).
// k_stem_norm: out = max(fl(fl(out - mean) * rstd), 0) in place.
// What they leave on the table is in DESIGN.md.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_encoder.h"
#include "conv_tile.hpp"

namespace bt {

constexpr int ST_NT = BT_ENC_CSTEM / 16, ST_WLD = conv_wld(BT_ENC_CSTEM);
constexpr int ST_KY = 7, ST_KX = 8, ST_ROWS = ST_KY * BT_ENC_CIMG * ST_KX;                       // 168 rows of the packed weight
constexpr int ST_HW = 2 * (CT_TW - 1) + ST_KX, ST_HH = 2 * (CT_TH - 1) + ST_KY;                  // 38 x 21
constexpr int ST_HALF = ST_HW / 2, ST_PART = BT_ENC_CIMG * ST_HH * ST_HALF;                      // 19 columns a part; 1197 floats
constexpr int ST_ODD = ((ST_PART + 15) / 32) * 32 + 16, ST_HALO = BT_ENC_CIMG * ST_HH * ST_HW;   // 1200; 2394 staged elements
static_assert(ST_NT == 4 && ST_ROWS == 168 && ST_HW == 38 && ST_HH == 21, "the stem's tile");
constexpr int ST_TPW = 3;                                                                       // tiles a workgroup takes
static_assert(ST_ODD >= ST_PART && ST_ODD % 32 == 16, "the odd part's LDS offset");

// ------------------------------------------------------------------------------------------------------------- k_stem_conv
// workgroup blockIdx.x takes tiles ST_TPW blockIdx.x .. of frame blockIdx.y, one after the other; part [F][tiles][64][2];
// rows16: wo % 4 == 0 and out 16-byte aligned, so a lane's four pixels of a row are stored as one float4
__global__ __launch_bounds__(CT_THREADS) void k_stem_conv(const ConvView X, const float *__restrict__ wp, const float *__restrict__ bias, int ho, int wo,
                                                          int tiles_x, int tiles, int rows16, float *__restrict__ out, double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float w_l[ST_ROWS * ST_WLD];          // [ky][c][kx][ST_WLD]
    __shared__ __attribute__((aligned(16))) float in_l[ST_ODD + ST_PART];         // even columns [c][row][19], then the odd ones
    static_assert(sizeof(float) * (ST_ROWS * ST_WLD + ST_ODD + ST_PART) <= 65536, "static LDS");
    static_assert((ST_ODD + ST_PART) * sizeof(float) >= (CT_THREADS / 64) * BT_ENC_CSTEM * 2 * sizeof(double), "the statistics reuse the halo's LDS");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
    const int f = blockIdx.y, t0 = blockIdx.x * ST_TPW, t1 = t0 + ST_TPW < tiles ? t0 + ST_TPW : tiles;
    const long long hwo = (long long)ho * wo;
    const float *xf = X.p + (long long)f * X.sf;

    // A tile's halo goes into registers (`fetch`) while the tile before it is multiplied, and reaches LDS (`stage`) when that
    // one is done.  Every load is unconditional: the address clamped into the image, the value dropped outside.
    constexpr int HN = (ST_HALO + CT_THREADS - 1) / CT_THREADS;
    float hreg[HN];
    auto fetch = [&](int t) __attribute__((always_inline)) {
        const int iy0 = 2 * (t / tiles_x) * CT_TH - 3, ix0 = 2 * (t % tiles_x) * CT_TW - 3;      // the halo's first input row and column
#pragma unroll
        for (int k = 0; k < HN; ++k) {
            const int idx = tid + k * CT_THREADS, ic = idx < ST_HALO ? idx : ST_HALO - 1;
            const int row = ic / ST_HW, hx = ic - row * ST_HW, c = row / ST_HH, hy = row - c * ST_HH;
            const int gy = iy0 + hy, gx = ix0 + hx;
            const bool in = hx < ST_HW - 1 && gy >= 0 && gy < X.h && gx >= 0 && gx < X.w;
            const int cy = gy < 0 ? 0 : (gy < X.h ? gy : X.h - 1), cx = gx < 0 ? 0 : (gx < X.w ? gx : X.w - 1);
            const float v = xf[c * X.sc + cy * X.sy + cx * X.sx];
            hreg[k] = in ? v : 0.0f;                             // zero padding of the image; the column of the zero weight
        }
    };
    auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < HN; ++k) {
            const int idx = tid + k * CT_THREADS;
            const int row = idx / ST_HW, hx = idx - row * ST_HW;
            if (idx < ST_HALO) in_l[((hx & 1) ? ST_ODD : 0) + row * ST_HALF + (hx >> 1)] = hreg[k];
        }
    };
    fetch(t0);
    tile_stage_rows<ST_ROWS, BT_ENC_CSTEM, 4>(w_l, wp, BT_ENC_CSTEM);            // resident for all of the workgroup's tiles

    // output x of tap kx reads halo column 2 x + kx: element x + kx / 2 of the even or of the odd part; kx = 4 g + q
    const float *a_l = in_l + ((q & 1) ? ST_ODD : 0) + (q >> 1) + 4 * wave * ST_HALF + l16, *b_l = w_l + q * ST_WLD + l16;
    for (int t = t0; t < t1; ++t) {
        __syncthreads();                                         // the tile before: its halo and its statistics are read
        stage();
        __syncthreads();
        if (t + 1 < t1) fetch(t + 1);                            // in flight while this tile is multiplied
        f32x4 acc[2][ST_NT], tot[2][ST_NT];
        tile_zero<ST_NT>(acc);
        tile_zero<ST_NT>(tot);
#pragma unroll
        for (int ky = 0; ky < ST_KY; ++ky) {
#pragma unroll
            for (int c = 0; c < BT_ENC_CIMG; ++c)
#pragma unroll
                for (int g = 0; g < ST_KX / 4; ++g) {
                    const float *ap = a_l + (c * ST_HH + ky) * ST_HALF + 2 * g;
                    tile_group<ST_NT>(ap[0], ap[2 * ST_HALF], b_l + ((ky * BT_ENC_CIMG + c) * ST_KX + 4 * g) * ST_WLD, acc);
                }
            tile_flush<ST_NT>(tot, acc);                         // a kernel row is complete: one rounded add into the total
        }
        __syncthreads();                                         // the halo is read: its LDS takes the statistics
        tile_store_stats<ST_NT, true, true>(tot, bias, out + (long long)f * BT_ENC_CSTEM * hwo, hwo, ho, wo, (t / tiles_x) * CT_TH, (t % tiles_x) * CT_TW,
                                            reinterpret_cast<double *>(in_l), part + ((long long)f * tiles + t) * BT_ENC_CSTEM * 2, rows16 != 0);
    }
}

// ------------------------------------------------------------------------------------------------------------- k_stem_norm
// out [F][64][n] holds raw and is normalised in place; the statistics [F][64].  V pixels a thread.
template <int V>
__global__ __launch_bounds__(256) void k_stem_norm(const float *__restrict__ mean, const float *__restrict__ rstd, long long n, float *out) {
    const long long p = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (p >= n) return;
    const long long fc = (long long)blockIdx.z * BT_ENC_CSTEM + blockIdx.y, base = fc * n + p;
    const float m = mean[fc], r = rstd[fc];
    float y[V];
    if constexpr (V == 4) {                                      // V == 4 only with n % 4 == 0 and a 16-byte aligned out
        const float4 t = *reinterpret_cast<const float4 *>(out + base);
        y[0] = t.x; y[1] = t.y; y[2] = t.z; y[3] = t.w;
    } else {
        y[0] = out[base];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) y[j] = norm_relu(y[j], m, r);
    if constexpr (V == 4) *reinterpret_cast<float4 *>(out + base) = float4{y[0], y[1], y[2], y[3]};
    else out[base] = y[0];
}

// the tiles' partials, then mean and rstd; no raw map (it is `out`); false when the sizes are refused
static bool stem_layout(long long F, long long h, long long w, ConvLayout *L) {
    return conv_layout(F, BT_ENC_CSTEM, conv_out(h, 2), conv_out(w, 2), 0, 1, 1, L);
}

}  // namespace bt

extern "C" size_t bt_encoder_stem_workspace_bytes(int64_t F, int64_t h_in, int64_t w_in) {
    bt::ConvLayout L;
    return bt::stem_layout(F, h_in, w_in, &L) ? L.bytes : 0;
}

extern "C" int bt_encoder_stem(const bt_encoder_level *x, const float *w_packed, const float *bias, int64_t c_out, int64_t F, void *workspace,
                               float *out, void *stream) {
    using namespace bt;
    if (!w_packed || !bias || !workspace || !out || level_invalid(x)) return BT_EINVAL;
    if (F < 1 || x->C < 1 || c_out < 1) return BT_EINVAL;
    if (((uintptr_t)w_packed & 15) || ((uintptr_t)workspace & 15)) return BT_EINVAL;
    if (c_out != BT_ENC_CSTEM || F > 65535 || level_check(x, BT_ENC_CIMG, F) != BT_OK) return BT_EUNSUPPORTED;
    ConvLayout L;
    if (!stem_layout(F, x->h, x->w, &L)) return BT_EUNSUPPORTED;

    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)workspace;
    float *mean = (float *)((char *)workspace + L.stat), *rstd = mean + L.stat_slot;
    const long long wo = conv_out(x->w, 2);
    const bool out16 = ((uintptr_t)out & 15) == 0;
    hipLaunchKernelGGL(k_stem_conv, dim3((unsigned)((L.tiles + ST_TPW - 1) / ST_TPW), (unsigned)F), dim3(CT_THREADS), 0, st, conv_view(*x), w_packed, bias,
                       (int)conv_out(x->h, 2), (int)wo, (int)conv_tiles_x(wo), (int)L.tiles, (int)(wo % 4 == 0 && out16), out, part);
    if (hipGetLastError() != hipSuccess) return BT_EHIP;
    if (!conv_stats_launch(st, part, L.tiles, BT_ENC_CSTEM, L.stat_slot, L.n, mean, rstd)) return BT_EHIP;
    return pointwise_launch(k_stem_norm<4>, k_stem_norm<1>, L.n % 4 == 0 && out16, L.n, BT_ENC_CSTEM, F, st, mean, rstd, L.n, out) ? BT_OK : BT_EHIP;
}
