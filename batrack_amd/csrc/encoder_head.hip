// encoder_head.hip — the feature encoder's head (include/batrack_encoder.h holds the specification): k_head_conv,
// k_head_norm_conv.
//
// k_head_conv is the 3 x 3 convolution 416 -> 256 over the VIRTUAL concatenation of the four pyramid levels, each resized to
// the output map (bilinear, align_corners): an implicit GEMM on v_mfma_f32_16x16x4_f32, k_embed_conv's tile once more
// (csrc/window_fmaps.hip).  Rows are output pixels, columns output channels, K = 9 taps x 416 input channels.
//   tile     a workgroup (4 waves) owns a 16 x 8 tile of output pixels of one frame and ONE HALF of the 256 columns
//            (blockIdx.z): wave v owns tile rows 2v and 2v + 1, each a 16-pixel MFMA row block: 2 x 8 accumulators of 4
//            registers.  All 256 columns in one wave would be 128 accumulator registers; two halves keep k_embed_conv's
//            budget (two workgroups a CU) at the price of sampling the halo tile twice.
//   K-chunk  8 input channels at a time (52 chunks; 64, 96, 128, 128 are multiples of 8, so a chunk lies in one level): their
//            18 x 10 halo tile is COMPUTED into LDS from the chunk's level — four taps and two weights per axis, which are
//            worked out once per tile for the 10 halo rows and 18 halo columns of each level and kept in LDS — and is zero
//            outside the output map (the padding is of the resized map); their 9 x 8 x 128 weights are staged beside it.
//   operands as k_embed_conv: A one ds_read_b32 from the halo tile at the tap's offset, B one from the weights; plane
//            stride 208 and weight row stride 144 are 16 mod 32.  A B fragment feeds both row blocks.
//   order    chunk, tap, group of four channels: fixed, the same for every pixel of every frame, whatever F is.  The MFMA is a
//            float32 fma chain; one chain over all 3744 products misses the reference's own float32 error by a factor of
//            four (measured), so every HC_FLUSH = 2 chunks (144 products) the accumulators are added into a second set and
//            start again from zero: 26 short chains and 26 adds.  128 accumulator registers after all, 182 VGPRs in all,
//            still two waves a SIMD (amdgpu_waves_per_eu keeps the allocator to that).
//   output   y2 = conv2 + bias2 as [F][256][h * w] planes in the workspace, and per (frame, tile, column) the float64 sum and
//            sum of squares of the tile's pixels: lane, then the four lane groups, then the four waves, always in that order.
//
// k_head_norm_conv reduces the tiles' partials of its frame in tile order (one thread per channel: every workgroup of a
// frame computes the same 256 means and reciprocal deviations), then normalises, clamps and multiplies: a workgroup owns 128
// consecutive pixels of one frame and all 128 output columns, wave v two 16-pixel row blocks; K = 256 in chunks of 32
// channels, whose normalised values and weights are staged in LDS.  Order: channel ascending, each chunk's chain added into
// the total when the chunk is done (as above), the bias last.
// What both leave on the table is in DESIGN.md.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_encoder.h"
#include "../../include/batrack_window.h"

namespace bt {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int HC_THREADS = 256, HC_TW = 16, HC_TH = 8, HC_HW = HC_TW + 2, HC_HH = HC_TH + 2, HC_HALO = HC_HW * HC_HH;
constexpr int HC_KC = BT_WINDOW_KCHUNK, HC_PL = 208, HC_COLS = 128, HC_WLD = 144, HC_CHUNKS = BT_ENC_CIN / HC_KC, HC_NT = HC_COLS / 16;
constexpr int HC_HALVES = BT_ENC_CMID / HC_COLS, HC_FLUSH = 2;
static_assert(HC_PL >= HC_HALO && HC_PL % 32 == 16 && HC_WLD >= HC_COLS && HC_WLD % 32 == 16, "LDS strides");
static_assert(HC_CHUNKS % HC_FLUSH == 0 && HC_CHUNKS * HC_KC == BT_ENC_CIN && HC_TH == 2 * (HC_THREADS / 64) && HC_HALVES * HC_COLS == BT_ENC_CMID, "tiling");
static_assert(BT_ENC_CA % HC_KC == 0 && BT_ENC_CB % HC_KC == 0 && BT_ENC_CC % HC_KC == 0 && BT_ENC_CD % HC_KC == 0, "a chunk lies in one level");
static_assert(BT_ENC_CA + BT_ENC_CB + BT_ENC_CC + BT_ENC_CD == BT_ENC_CIN, "the concatenation");
static_assert(9 * HC_KC * HC_WLD * sizeof(float) >= (HC_THREADS / 64) * HC_COLS * 2 * sizeof(double), "the statistics reuse the weights' LDS");

constexpr int NC_THREADS = 256, NC_PIX = 128, NC_KC = 32, NC_ZLD = 144, NC_WLD = 144, NC_NT = BT_ENC_COUT / 16;
static_assert(NC_THREADS == BT_ENC_CMID, "one thread per channel reduces the statistics");
static_assert(NC_PIX == 32 * (NC_THREADS / 64) && NC_ZLD >= NC_PIX && NC_ZLD % 32 == 16 && NC_WLD >= BT_ENC_COUT && NC_WLD % 32 == 16, "tiling");
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
__global__ __launch_bounds__(HC_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void k_head_conv(const HeadLevels L, const float *__restrict__ wp, const float *__restrict__ bias,
                                                         int h, int w, int tiles_x, float *__restrict__ ybuf, double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float w_l[9 * HC_KC * HC_WLD];       // [tap][channel of the chunk][HC_WLD]
    __shared__ float in_l[HC_KC * HC_PL];                                         // [channel of the chunk][halo pixel]
    __shared__ int ty_i[4][2][HC_HH], tx_i[4][2][HC_HW];                          // per level: the two source rows / columns
    __shared__ float ty_l[4][HC_HH], tx_l[4][HC_HW];                              // and the weight l1 of the second
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
    const int f = blockIdx.y, half = blockIdx.z, ty0 = (blockIdx.x / tiles_x) * HC_TH, tx0 = (blockIdx.x % tiles_x) * HC_TW;
    const long long hw = (long long)h * w;

    for (int i = tid; i < 4 * (HC_HH + HC_HW); i += HC_THREADS) {
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

    f32x4 acc[2][HC_NT], tot[2][HC_NT];                          // the running block of HC_FLUSH chunks, and the blocks before it
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int ct = 0; ct < HC_NT; ++ct) acc[r][ct] = tot[r][ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int chunk = 0; chunk < HC_CHUNKS; ++chunk) {
        __syncthreads();                                         // the previous chunk's reads are done (and the taps are written)
        const float4 *wsrc = reinterpret_cast<const float4 *>(wp + (size_t)chunk * 9 * HC_KC * BT_ENC_CMID + half * HC_COLS);
        for (int i = tid; i < 9 * HC_KC * (HC_COLS / 4); i += HC_THREADS) {
            const int row = i >> 5, c4 = i & 31;
            *reinterpret_cast<float4 *>(w_l + row * HC_WLD + c4 * 4) = wsrc[row * (BT_ENC_CMID / 4) + c4];
        }
        constexpr int E0 = BT_ENC_CA / HC_KC, E1 = E0 + BT_ENC_CB / HC_KC, E2 = E1 + BT_ENC_CC / HC_KC;
        const int lv = (chunk >= E0) + (chunk >= E1) + (chunk >= E2);
        const int c0 = (chunk - (lv == 0 ? 0 : (lv == 1 ? E0 : (lv == 2 ? E1 : E2)))) * HC_KC;
        const float *src = L.p[lv] + (long long)f * L.sf[lv] + (long long)c0 * L.sc[lv];
        const long long sc = L.sc[lv], sy = L.sy[lv], sx = L.sx[lv];
        for (int idx = tid; idx < HC_KC * HC_HALO; idx += HC_THREADS) {
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
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
            for (int s = 0; s < HC_KC / 4; ++s) {
                const float *ap = in_l + (4 * s + q) * HC_PL + (2 * wave + ky) * HC_HW + l16 + kx;
                const float a0 = ap[0], a1 = ap[HC_HW];
                const float *wr = w_l + (tap * HC_KC + 4 * s + q) * HC_WLD + l16;
#pragma unroll
                for (int ct = 0; ct < HC_NT; ++ct) {
                    const float b = wr[ct * 16];
                    acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][ct], 0, 0, 0);
                    acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][ct], 0, 0, 0);
                }
            }
        }
        if (chunk % HC_FLUSH == HC_FLUSH - 1) {                  // a block is complete: one rounded add into the total
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int ct = 0; ct < HC_NT; ++ct) {
                    tot[r][ct] += acc[r][ct];
                    acc[r][ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
        }
    }
    __syncthreads();                                             // the last chunk's weights are read: their LDS takes the statistics
    // register j of lane l is pixel 4 (l / 16) + j of the row block, column 16 ct + l % 16
    double *red = reinterpret_cast<double *>(w_l);               // [wave][column of the half][sum, sum of squares]
    float *yb = ybuf + ((long long)f * BT_ENC_CMID + half * HC_COLS) * hw;
#pragma unroll
    for (int ct = 0; ct < HC_NT; ++ct) {
        const int col = ct * 16 + l16;
        const float b = bias[half * HC_COLS + col];
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = ty0 + 2 * wave + r;
            float *yrow = yb + (long long)col * hw + (long long)y * w;
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
        if (q == 0) { red[(wave * HC_COLS + col) * 2] = s1; red[(wave * HC_COLS + col) * 2 + 1] = s2; }
    }
    __syncthreads();
    if (tid < HC_COLS) {
        double s1 = red[tid * 2], s2 = red[tid * 2 + 1];
        for (int v = 1; v < HC_THREADS / 64; ++v) { s1 += red[(v * HC_COLS + tid) * 2]; s2 += red[(v * HC_COLS + tid) * 2 + 1]; }
        double *pp = part + (((long long)f * gridDim.x + blockIdx.x) * BT_ENC_CMID + half * HC_COLS + tid) * 2;
        pp[0] = s1; pp[1] = s2;
    }
}

// ------------------------------------------------------------------------------------------------------- k_head_norm_conv
__global__ __launch_bounds__(NC_THREADS) void k_head_norm_conv(const float *__restrict__ ybuf, const double *__restrict__ part, int tiles,
                                                              const float *__restrict__ w3p, const float *__restrict__ bias3,
                                                              long long hw, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float w_l[NC_KC * NC_WLD];            // [channel of the chunk][output column]
    __shared__ float z_l[NC_KC * NC_ZLD];                                         // [channel of the chunk][pixel of the block]
    __shared__ float mean_l[BT_ENC_CMID], rstd_l[BT_ENC_CMID];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
    const int f = blockIdx.y;
    const long long p0 = (long long)blockIdx.x * NC_PIX;

    {
        const double *pp = part + ((long long)f * tiles * BT_ENC_CMID + tid) * 2;
        double s1 = 0.0, s2 = 0.0;
        for (int t = 0; t < tiles; ++t) { s1 += pp[(long long)t * BT_ENC_CMID * 2]; s2 += pp[(long long)t * BT_ENC_CMID * 2 + 1]; }
        const double n = (double)hw, mean = s1 / n;
        double var = s2 / n - mean * mean;
        var = var > 0.0 ? var : 0.0;
        mean_l[tid] = (float)mean;
        rstd_l[tid] = (float)(1.0 / sqrt(var + 1e-5));
    }

    f32x4 acc[2][NC_NT], tot[2][NC_NT];                          // the running chunk, and the chunks before it
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int ct = 0; ct < NC_NT; ++ct) acc[r][ct] = tot[r][ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const float *yb = ybuf + (long long)f * BT_ENC_CMID * hw;
    for (int chunk = 0; chunk < BT_ENC_CMID / NC_KC; ++chunk) {
        __syncthreads();                                         // the previous chunk's reads are done (and the statistics are written)
        const float4 *wsrc = reinterpret_cast<const float4 *>(w3p + (size_t)chunk * NC_KC * BT_ENC_COUT);
        for (int i = tid; i < NC_KC * (BT_ENC_COUT / 4); i += NC_THREADS) {
            const int row = i >> 5, c4 = i & 31;
            *reinterpret_cast<float4 *>(w_l + row * NC_WLD + c4 * 4) = wsrc[i];
        }
        for (int idx = tid; idx < NC_KC * NC_PIX; idx += NC_THREADS) {
            const int chl = idx / NC_PIX, p = idx - chl * NC_PIX, c = chunk * NC_KC + chl;
            float z = 0.0f;
            if (p0 + p < hw) {
                z = __fmul_rn(__fsub_rn(yb[(long long)c * hw + p0 + p], mean_l[c]), rstd_l[c]);
                z = z > 0.0f ? z : 0.0f;
            }
            z_l[chl * NC_ZLD + p] = z;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NC_KC / 4; ++s) {
            const float *ap = z_l + (4 * s + q) * NC_ZLD + 32 * wave + l16;
            const float a0 = ap[0], a1 = ap[16];
            const float *wr = w_l + (4 * s + q) * NC_WLD + l16;
#pragma unroll
            for (int ct = 0; ct < NC_NT; ++ct) {
                const float b = wr[ct * 16];
                acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][ct], 0, 0, 0);
                acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][ct], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)                              // the chunk is complete: one rounded add into the total
#pragma unroll
            for (int ct = 0; ct < NC_NT; ++ct) {
                tot[r][ct] += acc[r][ct];
                acc[r][ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
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

constexpr long long kEncI31 = 2147483647LL;

static long long enc_tiles(long long h, long long w) { return ((h + HC_TH - 1) / HC_TH) * ((w + HC_TW - 1) / HC_TW); }

// bytes of y2 [F][256][h * w] float32, then of the partials [F][tiles][256][2] float64; 0 when the sizes are refused
static size_t enc_workspace(long long F, long long h, long long w, size_t *part_offset) {
    if (F < 1 || h < 1 || w < 1 || F > kEncI31 || h > kEncI31 || w > kEncI31 || (__int128)F * BT_ENC_CMID * h * w > kEncI31) return 0;
    const size_t ybytes = ((size_t)F * BT_ENC_CMID * h * w * sizeof(float) + 15) & ~(size_t)15;
    if (part_offset) *part_offset = ybytes;
    return ybytes + (size_t)F * enc_tiles(h, w) * BT_ENC_CMID * 2 * sizeof(double);
}

// BT_OK when the level's view can be read with 32-bit-safe offsets
static int enc_level_check(const bt_encoder_level *l, long long C, long long F) {
    if (!l || !l->data || l->h < 1 || l->w < 1 || l->sf < 0 || l->sc < 0 || l->sy < 0 || l->sx < 0) return BT_EINVAL;
    if (l->C != C || l->h > kEncI31 || l->w > kEncI31 || l->sf > kEncI31 || l->sc > kEncI31 || l->sy > kEncI31 || l->sx > kEncI31) return BT_EUNSUPPORTED;
    if ((__int128)F * C * l->h * l->w > kEncI31
        || (__int128)(F - 1) * l->sf + (__int128)(C - 1) * l->sc + (__int128)(l->h - 1) * l->sy + (__int128)(l->w - 1) * l->sx > kEncI31)
        return BT_EUNSUPPORTED;
    return BT_OK;
}

}  // namespace bt

extern "C" size_t bt_encoder_head_workspace_bytes(int64_t F, int64_t h, int64_t w) { return bt::enc_workspace(F, h, w, nullptr); }

extern "C" int bt_encoder_head(const bt_encoder_level *a, const bt_encoder_level *b, const bt_encoder_level *c, const bt_encoder_level *d,
                               const float *w2_packed, const float *bias2, int64_t c_mid, const float *w3_packed, const float *bias3,
                               int64_t c_out, int64_t F, int64_t h, int64_t w, void *workspace, float *out, void *stream) {
    if (!a || !b || !c || !d || !w2_packed || !bias2 || !w3_packed || !bias3 || !workspace || !out) return BT_EINVAL;
    if (((uintptr_t)w2_packed & 15) || ((uintptr_t)w3_packed & 15) || ((uintptr_t)workspace & 15)) return BT_EINVAL;
    if (F < 1 || h < 1 || w < 1 || c_mid < 1 || c_out < 1) return BT_EINVAL;
    const bt_encoder_level *lv[4] = {a, b, c, d};
    const long long ch[4] = {BT_ENC_CA, BT_ENC_CB, BT_ENC_CC, BT_ENC_CD};
    for (int i = 0; i < 4; ++i)                                  // invalid arguments first, whatever level they are in
        if (bt::enc_level_check(lv[i], lv[i]->C, 1) == BT_EINVAL) return BT_EINVAL;
    if (c_mid != BT_ENC_CMID || c_out != BT_ENC_COUT || F > bt::kEncI31 || h > bt::kEncI31 || w > bt::kEncI31) return BT_EUNSUPPORTED;
    size_t part_offset = 0;
    if (bt::enc_workspace(F, h, w, &part_offset) == 0) return BT_EUNSUPPORTED;
    for (int i = 0; i < 4; ++i) {
        const int rc = bt::enc_level_check(lv[i], ch[i], F);
        if (rc != BT_OK) return rc;
    }
    const long long tiles_x = (w + bt::HC_TW - 1) / bt::HC_TW, tiles = bt::enc_tiles(h, w), hw = (long long)h * w;
    if (F > 65535 || tiles > bt::kEncI31) return BT_EUNSUPPORTED;
    bt::HeadLevels L;
    for (int i = 0; i < 4; ++i) {
        L.p[i] = lv[i]->data;
        L.sf[i] = lv[i]->sf; L.sc[i] = lv[i]->sc; L.sy[i] = lv[i]->sy; L.sx[i] = lv[i]->sx;
        L.hl[i] = (int)lv[i]->h; L.wl[i] = (int)lv[i]->w;
        L.scale_y[i] = h > 1 ? (float)(lv[i]->h - 1) / (float)(h - 1) : 0.0f;
        L.scale_x[i] = w > 1 ? (float)(lv[i]->w - 1) / (float)(w - 1) : 0.0f;
    }
    float *ybuf = (float *)workspace;
    double *part = (double *)((char *)workspace + part_offset);
    hipLaunchKernelGGL(bt::k_head_conv, dim3((unsigned)tiles, (unsigned)F, (unsigned)bt::HC_HALVES), dim3(bt::HC_THREADS), 0,
                       (hipStream_t)stream, L, w2_packed, bias2, (int)h, (int)w, (int)tiles_x, ybuf, part);
    if (hipGetLastError() != hipSuccess) return BT_EHIP;
    hipLaunchKernelGGL(bt::k_head_norm_conv, dim3((unsigned)((hw + bt::NC_PIX - 1) / bt::NC_PIX), (unsigned)F), dim3(bt::NC_THREADS), 0,
                       (hipStream_t)stream, (const float *)ybuf, (const double *)part, (int)tiles, w3_packed, bias3, hw, out);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
