// patch_gen.hip — the admission of a new frame for gfx950: the pooled gradient map of the image, the grid_grad candidates,
// their ranking per cell and the selected patches' rows with the disparity from the depth map and the colours
// (specification: include/batrack_patches.h).  Formulas: the reference's main/batrack.py:214-221 (__image_gradient_2),
// :280-325 (generate_patches, grid_grad), :917-934 (init_depth, 'dmap'), backend/altcorr/correlation.py:55-66 (patchify's
// blend), frontend/core/model_utils.py:75-158 (bilinear_sample2d).
//
// Two kernels, one launch each:
//   k_grad_pool       a workgroup per GP_TH x GP_TW tile of pooled cells.  uint8 rows whose bytes lie next to each other
//                     (HWC: 3*W bytes a row; planar: W bytes a channel row) are fetched as aligned 4-byte words into LDS,
//                     a wave per run; the gray sums of the (4*GP_TH+1) x (4*GP_TW+1) neighbourhood are then kept in LDS
//                     (16 bit for uint8 input, float32 otherwise), a lane per pooled cell adds its 16 roots in the
//                     reference's order and the tile's rows of g are written 128 bytes at a time.
//   k_patch_generate  C <= 64: a cell per wave, a lane per candidate, the rank by counting (v_j, j) < (v_i, i) over the
//                     wave's lanes; 64 < C <= 1024: a cell per workgroup, the scores in LDS.  The lanes whose rank is in
//                     the top gm then write their patch row.
// No atomics, no scratch: a call repeats bit for bit.  Everything here rounds every operation (contraction off), divides
// and takes roots correctly rounded: the file must not be built with a fast-math flag.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_patches.h"
#include "sample_taps.hpp"

#pragma clang fp contract(off)

namespace bt {

constexpr int GP_TH = 8, GP_TW = 32;            // pooled cells of a workgroup: one per thread
constexpr int GP_THREADS = GP_TH * GP_TW;
constexpr int GP_ROWS = 4 * GP_TH + 1;          // gray rows and columns the tile's roots read
constexpr int GP_COLS = 4 * GP_TW + 1;
constexpr int GP_LD = GP_COLS + 1;
constexpr int GP_ROW_WORDS = 99;                // staged words of a gray row: (3 + 3*GP_COLS + 3) / 4 = 98 as one run, 3 runs of (3 + GP_COLS + 3) / 4 = 33
enum { GP_ANY = 0, GP_HWC = 1, GP_PLANAR = 2 }; // how uint8 rows are fetched

struct GradArgs {
    const void *image;
    float *g;
    int64_t sc, sy, sx;
    int H, W, Hp, Wp, layout;
};

template <typename T>
__global__ __launch_bounds__(GP_THREADS) void k_grad_pool(GradArgs a) {
    constexpr bool U8 = std::is_same<T, uint8_t>::value;
    using S = typename std::conditional<U8, uint16_t, float>::type;     // 3 * 255 fits 16 bits
    __shared__ uint32_t s_stage[U8 ? GP_ROWS * GP_ROW_WORDS : 1];
    __shared__ S s_gray[GP_ROWS * GP_LD];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * GP_TH, j0 = blockIdx.x * GP_TW;
    const int y0 = 4 * i0 - 1, x0 = 4 * j0 - 1;                          // the tile's first gray row and column (-1: padding)
    const int xs = x0 < 0 ? 0 : x0, xe = x0 + GP_COLS < a.W ? x0 + GP_COLS : a.W;   // its columns inside the image
    const T *img = static_cast<const T *>(a.image);
    const int nruns = a.layout == GP_PLANAR ? 3 : 1, cap = GP_ROW_WORDS / nruns;
    if (U8 && a.layout != GP_ANY) {
        // a wave per run of adjacent bytes: the aligned words that cover it (a word that holds one byte of the row lies in
        // that byte's page)
        const int len = (xe - xs) * (a.layout == GP_HWC ? 3 : 1);
        for (int rr = tid >> 6; rr < GP_ROWS * nruns; rr += GP_THREADS / 64) {
            const int row = rr / nruns, ch = rr - row * nruns, y = y0 + row;
            if (y < 0 || y >= a.H || len <= 0) continue;
            const uint8_t *p = reinterpret_cast<const uint8_t *>(img) + (int64_t)y * a.sy + (int64_t)xs * a.sx + (int64_t)ch * a.sc;
            const unsigned lead = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
            const uint32_t *w = reinterpret_cast<const uint32_t *>(p - lead);
            const int nw = (int)(lead + len + 3) >> 2;
            for (int k = tid & 63; k < nw; k += 64) s_stage[rr * cap + k] = w[k];
        }
        __syncthreads();
    }
    for (int e = tid; e < GP_ROWS * GP_COLS; e += GP_THREADS) {
        const int row = e / GP_COLS, col = e - row * GP_COLS;
        const int y = y0 + row, x = x0 + col;
        S s = 0;
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
            if (U8 && a.layout != GP_ANY) {
                unsigned t = 0;
                const int step = a.layout == GP_HWC ? 3 : 1;
                for (int ch = 0; ch < 3; ++ch) {
                    const int run = a.layout == GP_HWC ? 0 : ch;
                    const uint8_t *p = reinterpret_cast<const uint8_t *>(img) + (int64_t)y * a.sy + (int64_t)xs * a.sx + (int64_t)run * a.sc;
                    const unsigned lead = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
                    const uint8_t *b = reinterpret_cast<const uint8_t *>(s_stage + (row * nruns + run) * cap);
                    t += b[lead + step * (x - xs) + (a.layout == GP_HWC ? ch : 0)];
                }
                s = (S)t;
            } else {
                const T *p = img + (int64_t)y * a.sy + (int64_t)x * a.sx;
                if (U8) s = (S)((unsigned)p[0] + (unsigned)p[a.sc] + (unsigned)p[2 * a.sc]);
                else    s = (S)(((float)p[0] + (float)p[a.sc]) + (float)p[2 * a.sc]);
            }
        }
        s_gray[row * GP_LD + col] = s;
    }
    __syncthreads();
    const int li = tid / GP_TW, lj = tid - li * GP_TW;
    const int i = i0 + li, j = j0 + lj;
    if (i < a.Hp && j < a.Wp) {
        float acc = 0.0f;
        for (int u = 0; u < 4; ++u)
            for (int v = 0; v < 4; ++v) {
                const int rr = 4 * li + u + 1, cc = 4 * lj + v + 1;      // gray (y, x) of lattice point (4i+u, 4j+v)
                float r;
                if (U8) {
                    const int s00 = s_gray[(rr - 1) * GP_LD + cc - 1];
                    const int dx = (int)s_gray[(rr - 1) * GP_LD + cc] - s00, dy = (int)s_gray[rr * GP_LD + cc - 1] - s00;
                    r = sqrtf((float)(dx * dx + dy * dy));
                } else {
                    const float s00 = s_gray[(rr - 1) * GP_LD + cc - 1];
                    const float dx = (float)s_gray[(rr - 1) * GP_LD + cc] - s00, dy = (float)s_gray[rr * GP_LD + cc - 1] - s00;
                    r = sqrtf(dx * dx + dy * dy);
                }
                acc = acc + r;
            }
        a.g[(int64_t)i * a.Wp + j] = acc * 0.0625f;
    }
}

struct PatchArgs {
    const float *g, *depth, *ux, *uy;
    const void *image;
    float *patches, *clr, *coords;
    uint8_t *colors;
    int32_t *sel;
    int64_t sc, sy, sx;
    int Hp, Wp, H, W, G, gm, C, Wg, Hg, dtype, rows;
};

// torch's sort order: a NaN above every number, -0 == +0
__device__ __forceinline__ bool pg_less(float a, float b) { return a < b || (b != b && a == a); }

// (v_j, j) < (v_i, i)
__device__ __forceinline__ bool pg_before(float vj, int j, float vi, int i) {
    return pg_less(vj, vi) || (!pg_less(vi, vj) && j < i);
}

__device__ __forceinline__ float pg_map_tap(const PatchArgs &a, float yy, float xx, float w, float acc) {
    if (xx >= 0.0f && xx <= (float)(a.Wp - 1) && yy >= 0.0f && yy <= (float)(a.Hp - 1))     // a NaN index is outside
        acc = acc + a.g[(int64_t)(int)yy * a.Wp + (int)xx] * w;
    return acc;
}

// F.grid_sample(g, (x_norm, y_norm), bilinear, align_corners=True, zeros)
__device__ __forceinline__ float pg_score(const PatchArgs &a, float xg, float yg) {
    const float xn = rintf(xg) / (float)(a.W - 1) * 2.0f - 1.0f;
    const float yn = (a.rows == BT_PATCH_ROWS_REFERENCE ? xn : rintf(yg)) / (float)(a.H - 1) * 2.0f - 1.0f;
    const float ix = ((xn + 1.0f) / 2.0f) * (float)(a.Wp - 1), iy = ((yn + 1.0f) / 2.0f) * (float)(a.Hp - 1);
    const float fx0 = floorf(ix), fy0 = floorf(iy), fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
    float v = 0.0f;
    v = pg_map_tap(a, fy0, fx0, (fx1 - ix) * (fy1 - iy), v);
    v = pg_map_tap(a, fy0, fx1, (ix - fx0) * (fy1 - iy), v);
    v = pg_map_tap(a, fy1, fx0, (fx1 - ix) * (iy - fy0), v);
    v = pg_map_tap(a, fy1, fx1, (ix - fx0) * (iy - fy0), v);
    return v;
}

__device__ __forceinline__ float pg_image_tap(const PatchArgs &a, int ch, int i, int j) {
    if (i < 0 || i >= a.H || j < 0 || j >= a.W) return 0.0f;
    const int64_t o = (int64_t)ch * a.sc + (int64_t)i * a.sy + (int64_t)j * a.sx;
    return a.dtype == BT_IMAGE_U8 ? (float)static_cast<const uint8_t *>(a.image)[o] : static_cast<const float *>(a.image)[o];
}

// (d) of the specification for output row p
__device__ __forceinline__ void pg_patch_row(const PatchArgs &a, int64_t p, int i, float xg, float yg) {
    // the coordinate grid: x plane j, y plane i at pixel (i, j), 0 outside
    const int i0 = floor_int(yg), j0 = floor_int(xg);
    const float dx = xg - floorf(xg), dy = yg - floorf(yg);
    const bool r0 = i0 >= 0 && i0 < a.H, r1 = i0 + 1 >= 0 && i0 + 1 < a.H, c0 = j0 >= 0 && j0 < a.W, c1 = j0 + 1 >= 0 && j0 + 1 < a.W;
    const float xj0 = (float)j0, xj1 = (float)(j0 + 1), yi0 = (float)i0, yi1 = (float)(i0 + 1);
    const float px = blend4(dx, dy, r0 && c0 ? xj0 : 0.0f, r0 && c1 ? xj1 : 0.0f, r1 && c0 ? xj0 : 0.0f, r1 && c1 ? xj1 : 0.0f);
    const float py = blend4(dx, dy, r0 && c0 ? yi0 : 0.0f, r0 && c1 ? yi0 : 0.0f, r1 && c0 ? yi1 : 0.0f, r1 && c1 ? yi1 : 0.0f);
    const float d = bilinear_clamped(a.depth, a.H, a.W, px, py);
    a.patches[3 * p] = px;
    a.patches[3 * p + 1] = py;
    a.patches[3 * p + 2] = 1.0f / clamp_min_1e2(d);
    if (a.coords) { a.coords[2 * p] = xg; a.coords[2 * p + 1] = yg; }
    if (a.sel) a.sel[p] = i;
    if (a.clr || a.colors) {
        const float xc = xg + 0.5f, yc = yg + 0.5f;
        const int ic = floor_int(yc), jc = floor_int(xc);
        const float ex = xc - floorf(xc), ey = yc - floorf(yc);
        for (int ch = 0; ch < 3; ++ch) {
            const float v = blend4(ex, ey, pg_image_tap(a, ch, ic, jc), pg_image_tap(a, ch, ic, jc + 1),
                                   pg_image_tap(a, ch, ic + 1, jc), pg_image_tap(a, ch, ic + 1, jc + 1));
            if (a.clr) a.clr[3 * p + ch] = v;
            if (a.colors) a.colors[3 * p + ch] = (uint8_t)(int)v;      // clr.to(torch.uint8): truncation
        }
    }
}

template <bool WAVE>
__global__ __launch_bounds__(WAVE ? 256 : 1024) void k_patch_generate(PatchArgs a) {
    __shared__ float s_v[WAVE ? 1 : BT_PATCH_MAX_CANDIDATES];
    const int64_t ncell = (int64_t)a.G * a.G;
    const int64_t cell = WAVE ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    const int i = WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const bool act = cell < ncell && i < a.C;
    float v = 0.0f, xg = 0.0f, yg = 0.0f;
    if (act) {
        const int cy = (int)(cell / a.G), cx = (int)(cell - (int64_t)cy * a.G);
        const float x = a.ux[cell * a.C + i] * 0.7f + 0.15f, y = a.uy[cell * a.C + i] * 0.7f + 0.15f;   // :291-292
        xg = x * (float)a.Wg + (float)(cx * a.Wg);                                                     // :301-302
        yg = y * (float)a.Hg + (float)(cy * a.Hg);
        v = pg_score(a, xg, yg);
    }
    int rank = 0;
    if (WAVE) {
        for (int j = 0; j < a.C; ++j) rank += pg_before(__shfl(v, j), j, v, i) ? 1 : 0;    // every lane of the wave walks the loop
    } else {
        if (i < a.C) s_v[i] = v;
        __syncthreads();
        for (int j = 0; j < a.C; ++j) rank += pg_before(s_v[j], j, v, i) ? 1 : 0;
    }
    if (act && rank >= a.C - a.gm) pg_patch_row(a, cell * a.gm + (rank - (a.C - a.gm)), i, xg, yg);
}

static int side_check(int64_t H, int64_t W) {
    if (H + 1 < 4 || W + 1 < 4) return BT_EINVAL;
    if (H > BT_PATCH_MAX_SIDE || W > BT_PATCH_MAX_SIDE) return BT_EUNSUPPORTED;
    return BT_OK;
}

}  // namespace bt

extern "C" int bt_image_gradient(const void *image, int32_t dtype, int64_t H, int64_t W, int64_t stride_c, int64_t stride_y,
                                 int64_t stride_x, float *g, void *stream) {
    if (!image || !g || (dtype != BT_IMAGE_U8 && dtype != BT_IMAGE_F32)) return BT_EINVAL;
    if (const int rc = bt::side_check(H, W)) return rc;
    bt::GradArgs a{image, g, stride_c, stride_y, stride_x, (int)H, (int)W, (int)((H + 1) / 4), (int)((W + 1) / 4), bt::GP_ANY};
    if (dtype == BT_IMAGE_U8) a.layout = (stride_x == 3 && stride_c == 1) ? bt::GP_HWC : (stride_x == 1 ? bt::GP_PLANAR : bt::GP_ANY);
    const dim3 grid((unsigned)((a.Wp + bt::GP_TW - 1) / bt::GP_TW), (unsigned)((a.Hp + bt::GP_TH - 1) / bt::GP_TH));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == BT_IMAGE_U8) hipLaunchKernelGGL(bt::k_grad_pool<uint8_t>, grid, dim3(bt::GP_THREADS), 0, st, a);
    else                      hipLaunchKernelGGL(bt::k_grad_pool<float>, grid, dim3(bt::GP_THREADS), 0, st, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

extern "C" int bt_patch_generate(const bt_patch_args *p, void *stream) {
    if (!p) return BT_EINVAL;
    if (!p->g || !p->image || !p->depth || !p->ux || !p->uy || !p->patches) return BT_EINVAL;
    if (p->dtype != BT_IMAGE_U8 && p->dtype != BT_IMAGE_F32) return BT_EINVAL;
    if (p->rows_mode != BT_PATCH_ROWS_REFERENCE && p->rows_mode != BT_PATCH_ROWS_IMAGE) return BT_EINVAL;
    if (p->H + 1 < 4 || p->W + 1 < 4 || p->G < 1 || p->gm < 1 || p->G > p->W || p->G > p->H) return BT_EINVAL;
    if (const int rc = bt::side_check(p->H, p->W)) return rc;
    if (p->Hp != (p->H + 1) / 4 || p->Wp != (p->W + 1) / 4) return BT_EINVAL;
    if (p->gm > BT_PATCH_MAX_CANDIDATES / 8) return BT_EUNSUPPORTED;
    bt::PatchArgs a{};
    a.g = p->g; a.depth = p->depth; a.ux = p->ux; a.uy = p->uy; a.image = p->image;
    a.patches = p->patches; a.clr = p->clr; a.coords = p->coords; a.colors = p->colors; a.sel = p->sel;
    a.sc = p->stride_c; a.sy = p->stride_y; a.sx = p->stride_x;
    a.Hp = (int)p->Hp; a.Wp = (int)p->Wp; a.H = (int)p->H; a.W = (int)p->W; a.G = (int)p->G; a.gm = (int)p->gm; a.C = 8 * a.gm;
    a.Wg = (int)(p->W / p->G); a.Hg = (int)(p->H / p->G); a.dtype = p->dtype; a.rows = p->rows_mode;
    const int64_t ncell = p->G * p->G;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.C <= 64) hipLaunchKernelGGL(bt::k_patch_generate<true>, dim3((unsigned)((ncell + 3) / 4)), dim3(256), 0, st, a);
    else           hipLaunchKernelGGL(bt::k_patch_generate<false>, dim3((unsigned)ncell), dim3((unsigned)((a.C + 63) / 64 * 64)), 0, st, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
