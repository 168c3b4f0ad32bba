// conv_tile.hpp — the implicit-GEMM convolution tile on v_mfma_f32_16x16x4_f32, once: k_embed_conv (csrc/window_fmaps.hip),
// k_head_conv and k_head_norm_conv (csrc/encoder_head.hip) and k_res_conv (csrc/encoder_trunk.hip) keep only how their
// operands reach LDS.  Rows of the GEMM are output pixels, columns output channels, K = taps x input channels.
//
// The tile.  A workgroup of CT_THREADS = 256 (4 waves) owns a CT_TW x CT_TH = 16 x 8 tile of output pixels of one frame and
// 16 NT output columns; wave v owns tile rows 2v and 2v + 1, each a 16-pixel MFMA row block: 2 x NT accumulators of 4
// registers.  Register j of lane l is pixel 4 (l / 16) + j of the row block, column 16 ct + l % 16.
// The K loop.  Chunks of CT_KC = 8 input channels: their halo tile (ConvGeom<S>: 18 x 10 input pixels at stride 1, 33 x 17 at
// stride 2, where a halo row is kept as its 17 even columns, then its 16 odd ones) is in LDS as [channel][halo pixel] with
// plane stride ConvGeom<S>::PL, their weights as [tap][channel][conv_wld(16 NT)].  Both strides are 16 mod 32, so that the two
// channel rows a 32-lane half reads fall on different banks.  Within a chunk the sum goes by tap, then by group of four
// channels; the MFMA is a float32 fma chain.
//
// tile_zero          acc = 0.
// tile_flush         tot += acc, acc = 0: one rounded float32 add per element.  k_head_conv and k_res_conv end a chain every
//                    CT_FLUSH = 2 chunks x 9 taps (144 products), k_head_norm_conv after every chunk of 32 channels.
// tile_group         one group of four channels: lane l holds pixel l % 16 of each row block and channel l / 16 of the group
//                    (a0, a1: one ds_read_b32 each) and reads the B fragment of channel l / 16, column 16 ct + l % 16 from `wr`.
//                    A B fragment feeds both row blocks: NT + 2 LDS reads per 2 NT MFMAs.
// tile_taps          a chunk: 9 taps x CT_KC / 4 groups from a halo tile and its weights.  Output x of tap kx reads halo column
//                    S x + kx: at stride 2 element x of the even part (kx = 0), x of the odd part (1) or x + 1 of the even
//                    part (2), at unit lane stride as at stride 1.  `centre(s, a0, a1)` is called with the centre tap's A
//                    fragments of group s: the 1 x 1 stride-2 shortcut's operands.
// tile_stage_rows    ROWS x COLS floats from rows `src_ld` floats apart into LDS rows of stride conv_wld(COLS), as float4:
//                    one load, one wait, one write a trip, or UNROLL loads in flight (the stride-2 k_res_conv: 3).
// tile_store_stats   raw = fl(tot + bias[column]) stored as [column][h * w] planes for the pixels inside the h x w map, and
//                    (STATS) per column the float64 sum and sum of squares of the float32 values STORED: lane (row block 0
//                    then 1, j ascending), then __shfl_xor 16 and 32, then the four waves in wave order through LDS; written
//                    as part_tile[column][2].  No atomics, and every (frame, tile, column) pair is written by its workgroup:
//                    the partials need no initialisation.  With STATS it contains a barrier: every thread of the workgroup
//                    calls it, `red` (LDS, 4 * 16 NT * 2 doubles) must not be in use by a thread that has not passed a
//                    barrier before the call, and is read until the next barrier after it.  VEC4 with `rows16` (w % 4 == 0 and
//                    16-byte aligned planes): a lane's four pixels of a row are stored as one float4; the same values and sums.
// tile_order_stats   the partials of one (frame, column) added in tile order; mean = sum / n, var = max(sumsq / n - mean^2, 0),
//                    rstd = 1 / sqrt(var + 1e-5), all float64, returned as floats.  A constant channel has an exact mean.
// norm_plain, norm_relu   fl(fl(v - mean) * rstd), and its maximum with 0: two rounded operations, never contracted.
//
// What surrounds the tile, once for the stem (encoder_stem.hip), the trunk (encoder_trunk.hip) and the head (encoder_head.hip):
// ConvView, conv_view   a strided [F, C, h, w] view by value in a kernel's arguments, and the one of a bt_encoder_level.
// conv_stats_launch     k_conv_stats (csrc/conv_stats.hip): one thread per (map, frame, channel) adds the tiles' partials in
//                       tile order (tile_order_stats) and stores mean and rstd as floats.
// pointwise_launch      a pointwise kernel over [F][C][n] planes, four pixels a thread or one: the argument list once.
// conv_layout           the workspace of a call: raw maps, then the tiles' partials, then mean and rstd sets.
// level_invalid, level_check   what every entry point refuses of a view, BT_EINVAL before BT_EUNSUPPORTED.
// kI31, view_fits_i31 (a strided [F, C, h, w] view within 32-bit-safe offsets), conv_out, conv_tiles_x, conv_tiles.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_encoder.h"

namespace bt {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CT_THREADS = 256, CT_TW = 16, CT_TH = 8, CT_KC = 8, CT_FLUSH = 2;
static_assert(CT_TH == 2 * (CT_THREADS / 64), "a wave owns two tile rows");

template <int S> struct ConvGeom {
    static constexpr int HW = S * (CT_TW - 1) + 3, HH = S * (CT_TH - 1) + 3, HALO = HW * HH;    // 18 x 10, 33 x 17
    static constexpr int EVEN = (HW + 1) / 2;                                                  // stride 2: the even columns first
    static constexpr int PL = ((HALO + 15) / 32) * 32 + 16;                                    // plane stride: 208, 592
    static_assert(PL >= HALO && PL % 32 == 16, "LDS plane stride");
};

constexpr int conv_wld(int cols) { return cols + 16; }                                         // weight row stride: 144 for 128 columns
static_assert(conv_wld(64) % 32 == 16 && conv_wld(96) % 32 == 16 && conv_wld(128) % 32 == 16, "LDS weight row stride");

template <int NT>
__device__ __forceinline__ void tile_zero(f32x4 (&acc)[2][NT]) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) acc[r][ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

template <int NT>
__device__ __forceinline__ void tile_flush(f32x4 (&tot)[2][NT], f32x4 (&acc)[2][NT]) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            tot[r][ct] += acc[r][ct];
            acc[r][ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
}

// wr: the group's weight row of this lane's channel, at column l % 16
template <int NT>
__device__ __forceinline__ void tile_group(float a0, float a1, const float *wr, f32x4 (&acc)[2][NT]) {
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
        const float b = wr[ct * 16];
        acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][ct], 0, 0, 0);
        acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][ct], 0, 0, 0);
    }
}

template <int S, int NT, class Centre>
__device__ __forceinline__ void tile_taps(const float *in_l, const float *w_l, f32x4 (&acc)[2][NT], Centre &&centre) {
    using G = ConvGeom<S>;
    constexpr int WLD = conv_wld(16 * NT);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, q = lane >> 4;
    const float *a_l = in_l + q * G::PL + S * 2 * wave * G::HW + l16, *b_l = w_l + q * WLD + l16;     // this lane's part of every address
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - 3 * ky;
        const int coff = S == 1 ? kx : (kx == 1 ? G::EVEN : (kx >> 1));
#pragma unroll
        for (int s = 0; s < CT_KC / 4; ++s) {
            const float *ap = a_l + 4 * s * G::PL + ky * G::HW + coff;
            const float a0 = ap[0], a1 = ap[S * G::HW];
            tile_group<NT>(a0, a1, b_l + (tap * CT_KC + 4 * s) * WLD, acc);
            if (tap == 4) centre(s, a0, a1);
        }
    }
}

template <int S, int NT>
__device__ __forceinline__ void tile_taps(const float *in_l, const float *w_l, f32x4 (&acc)[2][NT]) {
    tile_taps<S, NT>(in_l, w_l, acc, [](int, float, float) {});
}

template <int ROWS, int COLS, int UNROLL = 1>
__device__ __forceinline__ void tile_stage_rows(float *w_l, const float *__restrict__ src, int src_ld) {
    constexpr int C4 = COLS / 4, WLD = conv_wld(COLS);
    const float4 *s4 = reinterpret_cast<const float4 *>(src);
#pragma unroll UNROLL
    for (int i = threadIdx.x; i < ROWS * C4; i += CT_THREADS) {
        const int row = i / C4, c4 = i - row * C4;
        *reinterpret_cast<float4 *>(w_l + row * WLD + c4 * 4) = s4[row * (src_ld / 4) + c4];
    }
}

template <int NT, bool STATS, bool VEC4 = false>
__device__ __forceinline__ void tile_store_stats(const f32x4 (&tot)[2][NT], const float *__restrict__ bias, float *__restrict__ planes,
                                                 long long hw, int h, int w, int ty0, int tx0, double *red, double *__restrict__ part_tile,
                                                 bool rows16 = false) {
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
            if constexpr (VEC4) {
                if (rows16) {                                    // w % 4 == 0 and 16-byte planes: a lane's four pixels are one float4, all inside or all outside
                    const int x = tx0 + 4 * q;
                    if (y < h && x < w) {
                        float4 v4;
                        v4.x = __fadd_rn(tot[r][ct][0], b); v4.y = __fadd_rn(tot[r][ct][1], b);
                        v4.z = __fadd_rn(tot[r][ct][2], b); v4.w = __fadd_rn(tot[r][ct][3], b);
                        *reinterpret_cast<float4 *>(yrow + x) = v4;
                        if constexpr (STATS) {                   // the same adds in the same order as below
                            s1 += (double)v4.x; s2 += (double)v4.x * (double)v4.x;
                            s1 += (double)v4.y; s2 += (double)v4.y * (double)v4.y;
                            s1 += (double)v4.z; s2 += (double)v4.z * (double)v4.z;
                            s1 += (double)v4.w; s2 += (double)v4.w * (double)v4.w;
                        }
                    }
                    continue;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = tx0 + 4 * q + j;
                if (y < h && x < w) {
                    const float v = __fadd_rn(tot[r][ct][j], b);
                    yrow[x] = v;
                    if constexpr (STATS) {
                        s1 += (double)v;
                        s2 += (double)v * (double)v;
                    }
                }
            }
        }
        if constexpr (STATS) {
            s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
            s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
            if (q == 0) { red[(wave * COLS + col) * 2] = s1; red[(wave * COLS + col) * 2 + 1] = s2; }
        }
    }
    if constexpr (STATS) {
        __syncthreads();
        if (tid < COLS) {
            double s1 = red[tid * 2], s2 = red[tid * 2 + 1];
            for (int v = 1; v < CT_THREADS / 64; ++v) { s1 += red[(v * COLS + tid) * 2]; s2 += red[(v * COLS + tid) * 2 + 1]; }
            part_tile[tid * 2] = s1; part_tile[tid * 2 + 1] = s2;
        }
    }
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

__device__ __forceinline__ float norm_plain(float v, float mean, float rstd) { return __fmul_rn(__fsub_rn(v, mean), rstd); }

__device__ __forceinline__ float norm_relu(float v, float mean, float rstd) {
    const float z = norm_plain(v, mean, rstd);
    return z > 0.0f ? z : 0.0f;
}

struct ConvView {                // a strided [F, C, h, w] view, by value in the kernel's arguments
    const float *p;
    long long sf, sc, sy, sx;
    int h, w;
};

// ------------------------------------------------------------------------------------------------------------------ host
constexpr long long kI31 = 2147483647LL;

// whether every size, every stride, the element count and the farthest element offset of a strided [F, C, h, w] view are at
// most 2^31 - 1 (the callers have refused negative strides and sizes below 1 before)
inline bool view_fits_i31(long long F, long long C, long long h, long long w, long long sf, long long sc, long long sy, long long sx) {
    if (F > kI31 || C > kI31 || h > kI31 || w > kI31 || sf > kI31 || sc > kI31 || sy > kI31 || sx > kI31) return false;
    return (__int128)F * C * h * w <= kI31
        && (__int128)(F - 1) * sf + (__int128)(C - 1) * sc + (__int128)(h - 1) * sy + (__int128)(w - 1) * sx <= kI31;
}

inline long long conv_tiles_x(long long w) { return (w + CT_TW - 1) / CT_TW; }
inline long long conv_tiles(long long h, long long w) { return ((h + CT_TH - 1) / CT_TH) * conv_tiles_x(w); }
inline long long conv_out(long long n, long long stride) { return n < 1 ? 0 : (n - 1) / stride + 1; }      // 0: no such input size

inline ConvView conv_view(const bt_encoder_level &l) { return ConvView{l.data, l.sf, l.sc, l.sy, l.sx, (int)l.h, (int)l.w}; }

// a null view, a size below 1 or a negative stride: BT_EINVAL
inline bool level_invalid(const bt_encoder_level *l) {
    return !l || !l->data || l->h < 1 || l->w < 1 || l->sf < 0 || l->sc < 0 || l->sy < 0 || l->sx < 0;
}

// BT_OK when the level has C channels and its view of F frames can be read with 32-bit-safe offsets
inline int level_check(const bt_encoder_level *l, long long C, long long F) {
    if (level_invalid(l)) return BT_EINVAL;
    if (l->C != C || !view_fits_i31(F, C, l->h, l->w, l->sf, l->sc, l->sy, l->sx)) return BT_EUNSUPPORTED;
    return BT_OK;
}

// The workspace of a call on F frames of C channels of ho x wo output maps, as byte offsets: `raws` raw maps [F][C][n] float32
// from 0 (slot r at raw_slot * r floats), rounded up to 16 bytes; from `part` `parts` sets of the tiles' partials
// [F][tiles][C][2] float64; from `stat` `stats` means [F][C] float32, then as many rstds.  The head keeps 1 / 1 / 0, the stem
// 0 / 1 / 1 (its raw map is `out`), a block 2 or 3 of each.
struct ConvLayout {
    long long n, tiles, raw_slot, part_slot, stat_slot;
    size_t part, stat, bytes;
};

// false when the sizes are refused: one below 1 or above 2^31 - 1, or more than 2^31 - 1 elements in the raw maps (in one map
// when the call keeps none) or tiles.  The tile count cannot be what refuses: tiles <= ho * wo <= (2^31 - 1) / C whenever the
// element count passes.
inline bool conv_layout(long long F, long long C, long long ho, long long wo, int raws, int parts, int stats, ConvLayout *L) {
    if (F < 1 || ho < 1 || wo < 1 || F > kI31 || ho > kI31 || wo > kI31) return false;
    L->tiles = conv_tiles(ho, wo);
    if ((__int128)(raws ? raws : 1) * F * C * ho * wo > kI31 || L->tiles > kI31) return false;
    L->n = ho * wo; L->raw_slot = F * C * L->n; L->part_slot = F * L->tiles * C * 2; L->stat_slot = F * C;
    L->part = ((size_t)raws * L->raw_slot * sizeof(float) + 15) & ~(size_t)15;
    L->stat = L->part + (size_t)parts * L->part_slot * sizeof(double);
    L->bytes = L->stat + (size_t)stats * L->stat_slot * 2 * sizeof(float);
    return true;
}

// part [count / C][tiles][C][2] -> mean, rstd [count]; false when the launch fails (csrc/conv_stats.hip)
bool conv_stats_launch(hipStream_t st, const double *part, long long tiles, long long C, long long count, long long n, float *mean, float *rstd);

// k4 (four pixels a thread: the caller has checked n % 4 == 0 and the alignment of every plane) or k1 over n pixels of C
// channels of F frames, 256 threads a workgroup; false when the launch fails
template <class... A, class... B>
inline bool pointwise_launch(void (*k4)(A...), void (*k1)(A...), bool vec4, long long n, long long C, long long F, hipStream_t st, B... args) {
    hipLaunchKernelGGL(vec4 ? k4 : k1, dim3((unsigned)(((vec4 ? n / 4 : n) + 255) / 256), (unsigned)C, (unsigned)F), dim3(256), 0, st, args...);
    return hipGetLastError() == hipSuccess;
}

}  // namespace bt
