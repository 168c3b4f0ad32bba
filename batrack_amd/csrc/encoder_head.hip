// encoder_head.hip — the feature encoder's head (include/batrack_encoder.h holds the specification): k_head_conv,
// k_head_norm_conv.
//
// k_head_conv is the 3 x 3 convolution 416 -> 256 over the VIRTUAL concatenation of the four pyramid levels, each resized to
// the output map (bilinear, align_corners): an implicit GEMM on v_mfma_f32_16x16x4_f32 with the tile of csrc/conv_tile.hpp
// (stride 1), K = 9 taps x 416 input channels.
//   halves   a workgroup owns ONE HALF of the 256 columns (blockIdx.z).  All 256 columns in one wave would be 128
//            accumulator registers; two halves keep k_embed_conv's budget (two workgroups a CU) at the price of sampling the
//            halo tile twice.
//   K-chunk  8 input channels at a time (52 chunks; 64, 96, 128, 128 are multiples of 8, so a chunk lies in one level): their
//            18 x 10 halo tile is COMPUTED into LDS from the chunk's level — four taps and two weights per axis, which are
//            worked out once per tile for the 10 halo rows and 18 halo columns of each level and kept in LDS — and is zero
//            outside the output map (the padding is of the resized map); their 9 x 8 x 128 weights are staged beside it.
//   order    chunk, tap, group of four channels: fixed, the same for every pixel of every frame, whatever F is.  One fma
//            chain over all 3744 products misses the reference's own float32 error by a factor of four (measured), so every
//            CT_FLUSH = 2 chunks (144 products) the accumulators are added into a second set and start again from zero: 26
//            short chains and 26 adds.  128 accumulator registers after all, 182 VGPRs in all, still two waves a SIMD
//            (amdgpu_waves_per_eu keeps the allocator to that).
//   output   y2 = conv2 + bias2 as [F][256][h * w] planes in the workspace, and per (frame, tile, column) the float64 sum and
//            sum of squares of the tile's pixels (tile_store_stats).
//
// k_head_norm_conv reduces the tiles' partials of its frame in tile order (tile_order_stats, one thread per channel: every
// workgroup of a frame computes the same 256 means and reciprocal deviations), then normalises, clamps and multiplies: a
// workgroup owns 128 consecutive pixels of one frame and all 128 output columns, wave v two 16-pixel row blocks; K = 256 in
// chunks of 32 channels, whose normalised values and weights are staged in LDS.  Order: channel ascending (tile_group), each
// chunk's chain added into the total when the chunk is done (tile_flush), the bias last.
// What both leave on the table is in DESIGN.md.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_encoder.h"
#include "../../include/batrack_window.h"
#include "conv_tile.hpp"

namespace bt {

constexpr int HC_HW = ConvGeom<1>::HW, HC_HH = ConvGeom<1>::HH, HC_HALO = ConvGeom<1>::HALO, HC_PL = ConvGeom<1>::PL;
constexpr int HC_COLS = 128, HC_CHUNKS = BT_ENC_CIN / CT_KC, HC_NT = HC_COLS / 16, HC_HALVES = BT_ENC_CMID / HC_COLS;
static_assert(CT_KC == BT_WINDOW_KCHUNK && HC_CHUNKS % CT_FLUSH == 0 && HC_CHUNKS * CT_KC == BT_ENC_CIN && HC_HALVES * HC_COLS == BT_ENC_CMID, "tiling");
static_assert(BT_ENC_CA % CT_KC == 0 && BT_ENC_CB % CT_KC == 0 && BT_ENC_CC % CT_KC == 0 && BT_ENC_CD % CT_KC == 0, "a chunk lies in one level");
static_assert(BT_ENC_CA + BT_ENC_CB + BT_ENC_CC + BT_ENC_CD == BT_ENC_CIN, "the concatenation");
static_assert(9 * CT_KC * conv_wld(HC_COLS) * sizeof(float) >= (CT_THREADS / 64) * HC_COLS * 2 * sizeof(double), "the statistics reuse the weights' LDS");

constexpr int NC_PIX = 128, NC_KC = 32, NC_ZLD = conv_wld(NC_PIX), NC_WLD = conv_wld(BT_ENC_COUT), NC_NT = BT_ENC_COUT / 16;
static_assert(CT_THREADS == BT_ENC_CMID, "one thread per channel reduces the statistics");
static_assert(NC_PIX == 32 * (CT_THREADS / 64), "tiling");
static_assert(BT_ENC_CMID % NC_KC == 0 && NC_KC % 4 == 0, "K chunks");

struct HeadLevels {              // the four levels, by value in the kernel's arguments
    const float *p[4];
    long long sf[4], sc[4], sy[4], sx[4];
    int hl[4], wl[4];
    float scale_y[4], scale_x[4];
};

// torch's align_corners source index: src = scale * o, i0 = min((int)src, n - 1), i1 = min(i0 + 1, n - 1), l1 = src - i0
__device__ __forceinline__ void resize_tap(float scale, int o, int n_in, int &i0, int &i1, float &l1) {
    const float src = __fmul_rn(scale, (float)o);
    i0 = (int)src;
    i0 = i0 < n_in - 1 ? i0 : n_in - 1;
    i1 = i0 + 1 < n_in - 1 ? i0 + 1 : n_in - 1;
    l1 = __fsub_rn(src, (float)i0);
}

// ------------------------------------------------------------------------------------------------------------ k_head_conv
__global__ __launch_bounds__(CT_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void k_head_conv(const HeadLevels L, const float *__restrict__ wp, const float *__restrict__ bias,
                                                         int h, int w, int tiles_x, float *__restrict__ ybuf, double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float w_l[9 * CT_KC * conv_wld(HC_COLS)];       // [tap][channel of the chunk][144]
    __shared__ float in_l[CT_KC * HC_PL];                                         // [channel of the chunk][halo pixel]
    __shared__ int ty_i[4][2][HC_HH], tx_i[4][2][HC_HW];                          // per level: the two source rows / columns
    __shared__ float ty_l[4][HC_HH], tx_l[4][HC_HW];                              // and the weight l1 of the second
    const int tid = threadIdx.x;
    const int f = blockIdx.y, half = blockIdx.z, ty0 = (blockIdx.x / tiles_x) * CT_TH, tx0 = (blockIdx.x % tiles_x) * CT_TW;
    const long long hw = (long long)h * w;

    for (int i = tid; i < 4 * (HC_HH + HC_HW); i += CT_THREADS) {
        const int lv = i / (HC_HH + HC_HW), r = i - lv * (HC_HH + HC_HW);
        int i0, i1;
        float l1;
        if (r < HC_HH) {                                         // a halo row; one outside the map is never sampled
            int o = ty0 + r - 1;
            o = o < 0 ? 0 : (o > h - 1 ? h - 1 : o);
            resize_tap(L.scale_y[lv], o, L.hl[lv], i0, i1, l1);
            ty_i[lv][0][r] = i0; ty_i[lv][1][r] = i1; ty_l[lv][r] = l1;
        } else {
            int o = tx0 + (r - HC_HH) - 1;
            o = o < 0 ? 0 : (o > w - 1 ? w - 1 : o);
            resize_tap(L.scale_x[lv], o, L.wl[lv], i0, i1, l1);
            tx_i[lv][0][r - HC_HH] = i0; tx_i[lv][1][r - HC_HH] = i1; tx_l[lv][r - HC_HH] = l1;
        }
    }

    f32x4 acc[2][HC_NT], tot[2][HC_NT];                          // the running block of CT_FLUSH chunks, and the blocks before it
    tile_zero<HC_NT>(acc);
    tile_zero<HC_NT>(tot);

    for (int chunk = 0; chunk < HC_CHUNKS; ++chunk) {
        __syncthreads();                                         // the previous chunk's reads are done (and the taps are written)
        tile_stage_rows<9 * CT_KC, HC_COLS>(w_l, wp + (size_t)chunk * 9 * CT_KC * BT_ENC_CMID + half * HC_COLS, BT_ENC_CMID);
        constexpr int E0 = BT_ENC_CA / CT_KC, E1 = E0 + BT_ENC_CB / CT_KC, E2 = E1 + BT_ENC_CC / CT_KC;
        const int lv = (chunk >= E0) + (chunk >= E1) + (chunk >= E2);
        const int c0 = (chunk - (lv == 0 ? 0 : (lv == 1 ? E0 : (lv == 2 ? E1 : E2)))) * CT_KC;
        const float *src = L.p[lv] + (long long)f * L.sf[lv] + (long long)c0 * L.sc[lv];
        const long long sc = L.sc[lv], sy = L.sy[lv], sx = L.sx[lv];
        for (int idx = tid; idx < CT_KC * HC_HALO; idx += CT_THREADS) {
            const int chl = idx / HC_HALO, p = idx - chl * HC_HALO, hy = p / HC_HW, hx = p - hy * HC_HW;
            const int gy = ty0 + hy - 1, gx = tx0 + hx - 1;
            float v = 0.0f;                                      // zero padding of the resized map
            if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
                const float *s = src + chl * sc;
                const long long y0 = ty_i[lv][0][hy] * sy, y1 = ty_i[lv][1][hy] * sy, x0 = tx_i[lv][0][hx] * sx, x1 = tx_i[lv][1][hx] * sx;
                const float l1y = ty_l[lv][hy], l1x = tx_l[lv][hx], l0y = __fsub_rn(1.0f, l1y), l0x = __fsub_rn(1.0f, l1x);
                const float top = __fadd_rn(__fmul_rn(l0x, s[y0 + x0]), __fmul_rn(l1x, s[y0 + x1]));
                const float bot = __fadd_rn(__fmul_rn(l0x, s[y1 + x0]), __fmul_rn(l1x, s[y1 + x1]));
                v = __fadd_rn(__fmul_rn(l0y, top), __fmul_rn(l1y, bot));
            }
            in_l[chl * HC_PL + p] = v;
        }
        __syncthreads();
        tile_taps<1, HC_NT>(in_l, w_l, acc);
        if (chunk % CT_FLUSH == CT_FLUSH - 1) tile_flush<HC_NT>(tot, acc);   // a block is complete: one rounded add into the total
    }
    __syncthreads();                                             // the last chunk's weights are read: their LDS takes the statistics
    const long long col0 = (long long)f * BT_ENC_CMID + half * HC_COLS;     // the half's first column, among the frame's
    tile_store_stats<HC_NT, true>(tot, bias + half * HC_COLS, ybuf + col0 * hw, hw, h, w, ty0, tx0, reinterpret_cast<double *>(w_l),
                                  part + (((long long)f * gridDim.x + blockIdx.x) * BT_ENC_CMID + half * HC_COLS) * 2);
}

// ------------------------------------------------------------------------------------------------------- k_head_norm_conv
__global__ __launch_bounds__(CT_THREADS) void k_head_norm_conv(const float *__restrict__ ybuf, const double *__restrict__ part, int tiles,
                                                              const float *__restrict__ w3p, const float *__restrict__ bias3,
                                                              long long hw, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float w_l[NC_KC * NC_WLD];            // [channel of the chunk][output column]
    __shared__ float z_l[NC_KC * NC_ZLD];                                         // [channel of the chunk][pixel of the block]
    __shared__ float mean_l[BT_ENC_CMID], rstd_l[BT_ENC_CMID];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
    const int f = blockIdx.y;
    const long long p0 = (long long)blockIdx.x * NC_PIX;

    // the partials begin 16-byte aligned (bt_encoder_head refuses a workspace that is not, and conv_layout rounds the
    // bytes of y2 before them to 16), and a (tile, channel) pair is 16 bytes: tile_order_stats' double2 loads are legal
    tile_order_stats(part + ((long long)f * tiles * BT_ENC_CMID + tid) * 2, (long long)BT_ENC_CMID * 2, tiles, (double)hw, mean_l[tid], rstd_l[tid]);

    f32x4 acc[2][NC_NT], tot[2][NC_NT];                          // the running chunk, and the chunks before it
    tile_zero<NC_NT>(acc);
    tile_zero<NC_NT>(tot);

    const float *yb = ybuf + (long long)f * BT_ENC_CMID * hw;
    for (int chunk = 0; chunk < BT_ENC_CMID / NC_KC; ++chunk) {
        __syncthreads();                                         // the previous chunk's reads are done (and the statistics are written)
        tile_stage_rows<NC_KC, BT_ENC_COUT>(w_l, w3p + (size_t)chunk * NC_KC * BT_ENC_COUT, BT_ENC_COUT);
        for (int idx = tid; idx < NC_KC * NC_PIX; idx += CT_THREADS) {
            const int chl = idx / NC_PIX, p = idx - chl * NC_PIX, c = chunk * NC_KC + chl;
            float z = 0.0f;
            if (p0 + p < hw) z = norm_relu(yb[(long long)c * hw + p0 + p], mean_l[c], rstd_l[c]);
            z_l[chl * NC_ZLD + p] = z;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NC_KC / 4; ++s) {
            const float *ap = z_l + (4 * s + q) * NC_ZLD + 32 * wave + l16;
            tile_group<NC_NT>(ap[0], ap[16], w_l + (4 * s + q) * NC_WLD + l16, acc);
        }
        tile_flush<NC_NT>(tot, acc);                             // the chunk is complete: one rounded add into the total
    }
    // register j of lane l is pixel 4 (l / 16) + j of the row block, column 16 ct + l % 16
    float *ob = out + (long long)f * BT_ENC_COUT * hw;
#pragma unroll
    for (int ct = 0; ct < NC_NT; ++ct) {
        const int col = ct * 16 + l16;
        const float b = bias3[col];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long p = p0 + 32 * wave + 16 * r + 4 * q + j;
                if (p < hw) ob[(long long)col * hw + p] = __fadd_rn(tot[r][ct][j], b);
            }
    }
}

// y2 [F][256][h * w] float32, then the partials [F][tiles][256][2] float64; no statistics (k_head_norm_conv reduces in-kernel)
static bool head_layout(long long F, long long h, long long w, ConvLayout *L) { return conv_layout(F, BT_ENC_CMID, h, w, 1, 1, 0, L); }

}  // namespace bt

extern "C" size_t bt_encoder_head_workspace_bytes(int64_t F, int64_t h, int64_t w) {
    bt::ConvLayout L;
    return bt::head_layout(F, h, w, &L) ? L.bytes : 0;
}

extern "C" int bt_encoder_head(const bt_encoder_level *a, const bt_encoder_level *b, const bt_encoder_level *c, const bt_encoder_level *d,
                               const float *w2_packed, const float *bias2, int64_t c_mid, const float *w3_packed, const float *bias3,
                               int64_t c_out, int64_t F, int64_t h, int64_t w, void *workspace, float *out, void *stream) {
    if (!a || !b || !c || !d || !w2_packed || !bias2 || !w3_packed || !bias3 || !workspace || !out) return BT_EINVAL;
    if (((uintptr_t)w2_packed & 15) || ((uintptr_t)w3_packed & 15) || ((uintptr_t)workspace & 15)) return BT_EINVAL;
    if (F < 1 || h < 1 || w < 1 || c_mid < 1 || c_out < 1) return BT_EINVAL;
    const bt_encoder_level *lv[4] = {a, b, c, d};
    const long long ch[4] = {BT_ENC_CA, BT_ENC_CB, BT_ENC_CC, BT_ENC_CD};
    for (int i = 0; i < 4; ++i)                                  // invalid arguments first, whatever level they are in
        if (bt::level_invalid(lv[i])) return BT_EINVAL;
    bt::ConvLayout W;
    if (c_mid != BT_ENC_CMID || c_out != BT_ENC_COUT || F > 65535 || !bt::head_layout(F, h, w, &W)) return BT_EUNSUPPORTED;
    for (int i = 0; i < 4; ++i)
        if (bt::level_check(lv[i], ch[i], F) != BT_OK) return BT_EUNSUPPORTED;
    bt::HeadLevels L;
    for (int i = 0; i < 4; ++i) {
        const bt::ConvView v = bt::conv_view(*lv[i]);
        L.p[i] = v.p;
        L.sf[i] = v.sf; L.sc[i] = v.sc; L.sy[i] = v.sy; L.sx[i] = v.sx;
        L.hl[i] = v.h; L.wl[i] = v.w;
        L.scale_y[i] = h > 1 ? (float)(lv[i]->h - 1) / (float)(h - 1) : 0.0f;
        L.scale_x[i] = w > 1 ? (float)(lv[i]->w - 1) / (float)(w - 1) : 0.0f;
    }
    float *ybuf = (float *)workspace;
    double *part = (double *)((char *)workspace + W.part);
    hipLaunchKernelGGL(bt::k_head_conv, dim3((unsigned)W.tiles, (unsigned)F, (unsigned)bt::HC_HALVES), dim3(bt::CT_THREADS), 0,
                       (hipStream_t)stream, L, w2_packed, bias2, (int)h, (int)w, (int)bt::conv_tiles_x(w), ybuf, part);
    if (hipGetLastError() != hipSuccess) return BT_EHIP;
    hipLaunchKernelGGL(bt::k_head_norm_conv, dim3((unsigned)((W.n + bt::NC_PIX - 1) / bt::NC_PIX), (unsigned)F), dim3(bt::CT_THREADS), 0,
                       (hipStream_t)stream, (const float *)ybuf, (const double *)part, (int)W.tiles, w3_packed, bias3, W.n, out);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
