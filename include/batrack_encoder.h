/* batrack_encoder.h — C ABI of the feature encoder: its head (bt_encoder_head, below), one residual block of its trunk
 * layer1..4 (bt_res_block, specified before its declaration) and its stem conv1 7 x 7, norm1, relu1 (bt_encoder_stem,
 * specified before its declaration).
 *
 * The head (the reference's main/frontend/core/cotracker/blocks.py:241-273,
 * the last third of `BasicEncoder.forward` with norm_fn = "instance" and shallow = False): the four pyramid levels resized
 * to the output map, their concatenation convolved 3 x 3 from 416 to 256 channels, the instance normalisation, the ReLU and
 * the 1 x 1 convolution to 128 channels.  Neither the resized copies nor the concatenation is ever in memory: the
 * convolution samples the four small maps while it stages its input.
 *
 * Inference only, float32.  The levels a, b, c, d have BT_ENC_CA .. BT_ENC_CD = 64, 96, 128, 128 channels; the virtual
 * concatenation has BT_ENC_CIN = 416 in that order, conv2 gives BT_ENC_CMID = 256 and conv3 BT_ENC_COUT = 128.
 *
 * bt_encoder_head.  For every frame f < F, output pixel (y, x) of the h x w map:
 *
 *   resize (F.interpolate(mode = "bilinear", align_corners = True)), per level l of size hl x wl, per axis with output
 *   index o, n_in = the level's size and n_out = the output's:
 *     scale = (float)(n_in - 1) / (float)(n_out - 1), one float32 division, or 0 when n_out == 1
 *     src = scale * o;   i0 = min((int)src, n_in - 1);   i1 = min(i0 + 1, n_in - 1);   l1 = src - i0;   l0 = 1 - l1
 *     r[f, c, y, x] = l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11),   v_jk = level[f, c, i_j(y), i_k(x)],
 *   the element of level l at f * sf + c * sc + iy * sy + ix * sx (strided views, read in place).  A level whose size equals
 *   the output's has l1 = 0 everywhere and is reproduced exactly.  Every level may have any size >= 1 x 1.
 *
 *   conv2:  y2[f, m, y, x] = bias2[m] + sum over taps (ky, kx) in 3 x 3 and channels c < 416 of
 *     W2[m, c, ky, kx] * r[f, c, y + ky - 1, x + kx - 1],   a tap outside the h x w map contributing 0: the zero padding is
 *   of the RESIZED map, not of the sources.  Summed on v_mfma_f32_16x16x4_f32 in the kernel's fixed order (channel chunks of
 *   BT_WINDOW_KCHUNK = 8, then taps, then groups of 4 channels; csrc/encoder_head.hip), as 26 fma chains of two chunks (144
 *   products) each, every chain added to the total when it ends, the bias added last.
 *
 *   statistics, per (f, m) over the n = h * w pixels, in float64: sum and sum of squares of y2 (as stored, in float32), one
 *   partial per 16 x 8 tile in the workspace, the partials added in tile order.  No floating-point atomics.
 *     mean = sum / n;   var = max(sumsq / n - mean * mean, 0);   rstd = 1 / sqrt(var + 1e-5)      (biased variance, float64)
 *     z[f, m, y, x] = max((y2 - (float)mean) * (float)rstd, 0)                                     (float32)
 *   A constant channel (variance 0) has an exact mean, so z is exactly 0 there.
 *
 *   conv3:  out[f, o, y, x] = bias3[o] + sum over m < 256 of z[f, m, y, x] * W3[o, m], a 256-deep product on the same MFMA,
 *   m ascending, as 8 fma chains of 32 channels each added to the total when it ends, the bias added last.
 *
 * `w2_packed` is W2 repacked as [52][9][8][256]: w2_packed[c / 8][3 ky + kx][c % 8][m] = W2[m][c][ky][kx]; `w3_packed` is
 * [256][128]: w3_packed[m][o] = W3[o][m].  Both 16-byte aligned.  out is a contiguous [F, 128, h, w] (possibly a slice of a
 * larger buffer), the layout bt_embed_conv reads.
 *
 * Two launches, no host read.  The order of every sum is fixed and the same for every pixel of every frame, whatever F is:
 * a call repeats bit for bit, and frame f of a call on F frames has the bits of a call on that frame alone.
 *
 * workspace: bt_encoder_head_workspace_bytes(F, h, w) bytes (0 when the sizes are refused), 16-byte aligned.  It holds y2 and
 * the partial statistics; every byte that is read is written first, so it needs NO initialisation and may hold anything on
 * entry.  Two calls in flight must not share one.
 *
 * The four bt_encoder_level structures are read on the HOST during the call; every other pointer, and each level's `data`,
 * is a DEVICE pointer; `stream` is a hipStream_t as void*.  The library allocates nothing and never throws.
 * Returns
 *   BT_EINVAL        a null pointer; F, h, w or a level's height or width below 1; a negative stride; a packed weight or a
 *                    workspace that is not 16-byte aligned;
 *   BT_EUNSUPPORTED  channel counts other than 64 / 96 / 128 / 128 -> 256 -> 128; a size, a stride, an element offset of a
 *                    level's view or an element count (F * 256 * h * w) above 2^31 - 1; F above 65535 (the grid's second
 *                    dimension) or more than 2^31 - 1 tiles;
 *   BT_OK            otherwise;   BT_EHIP if a launch fails.
 * Every refusal happens before any HIP call. */
#ifndef BATRACK_ENCODER_H
#define BATRACK_ENCODER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BT_ENC_CA 64
#define BT_ENC_CB 96
#define BT_ENC_CC 128
#define BT_ENC_CD 128
#define BT_ENC_CIN 416           /* 64 + 96 + 128 + 128: w2_packed is [416 / 8][9][8][256] */
#define BT_ENC_CMID 256
#define BT_ENC_COUT 128

/* one pyramid level: a strided view [F, C, h, w] of float32, element (f, c, y, x) at f * sf + c * sc + y * sy + x * sx */
typedef struct bt_encoder_level {
    const float *data;
    int64_t C, h, w;
    int64_t sf, sc, sy, sx;
} bt_encoder_level;

size_t bt_encoder_head_workspace_bytes(int64_t F, int64_t h, int64_t w);

int bt_encoder_head(const bt_encoder_level *a, const bt_encoder_level *b, const bt_encoder_level *c, const bt_encoder_level *d,
                    const float *w2_packed, const float *bias2, int64_t c_mid, const float *w3_packed, const float *bias3,
                    int64_t c_out, int64_t F, int64_t h, int64_t w, void *workspace, float *out, void *stream);

/* bt_res_block — one `ResidualBlock` (blocks.py:16-75, norm_fn = "instance") of layer1..4.  Inference only, float32.
 * c_in, c_out in {64, 96, 128}; stride 1 (c_in == c_out, no shortcut convolution) or 2.  x is a strided view [F, c_in, h, w]
 * read in place; ho = (h - 1) / stride + 1, wo likewise; out is a contiguous [F, c_out, ho, wo].
 *
 *   raw1 = conv1(x) + b1:   3 x 3, zero padding 1, stride `stride`: output (y, x) has its centre tap at input
 *     (stride * y, stride * x).  Summed on v_mfma_f32_16x16x4_f32 in k_head_conv's order: chunks of 8 input channels ascending,
 *     then tap 3 ky + kx, then group of four channels; the fma chain is added into the total and starts again every two
 *     chunks (144 products); the bias is added last.
 *   rawd = downsample[0](x) + bd (stride 2 only):   1 x 1, stride 2, no padding: ONE fma chain over the c_in products in
 *     channel order, the bias last.
 *   statistics of raw1 (and rawd), per (frame, channel) over the n = ho * wo pixels: as the head's (float64 sum and sum of
 *     squares of the stored float32 values, one partial per 16 x 8 tile, added in tile order; no floating-point atomics);
 *     mean = sum / n; var = max(sumsq / n - mean^2, 0); rstd = 1 / sqrt(var + 1e-5) in float64, stored as floats m, r.
 *   raw2 = conv2(z1) + b2, z1 = max(fl(fl(raw1 - m1) * r1), 0):   3 x 3, stride 1, zero padding of z1 (NOT of raw1): a tap
 *     outside the map contributes 0.  z1 is never in memory.  The same order of sums; then raw2's statistics m2, r2.
 *   out = max(fl(s + max(fl(fl(raw2 - m2) * r2), 0)), 0),   s = x (stride 1) or fl(fl(rawd - md) * rd) (stride 2: norm3, no ReLU).
 *   A constant channel has an exact mean, so its normalised values are exactly 0.
 *
 * Packed weights, all 16-byte aligned: w1[c / 8][3 ky + kx][c % 8][m] = conv1.weight[m][c][ky][kx], [c_in / 8][9][8][c_out];
 * w2 likewise from conv2, [c_out / 8][9][8][c_out]; wd[c][m] = downsample[0].weight[m][c][0][0], [c_in][c_out]; wd and bd are
 * NULL exactly when stride is 1.
 *
 * Five launches (convolution, statistics, convolution, statistics, join), no host read.  The order of every sum is fixed:
 * a call repeats bit for bit, and frame f of F frames has the bits of that frame alone.
 *
 * workspace: bt_res_block_workspace_bytes(F, c_out, h, w, stride) bytes (0 when refused), 16-byte aligned: raw1, rawd, raw2,
 * the tiles' partials and the statistics.  Every byte that is read is written first: it needs NO initialisation.
 * `x` and `blk` are read on the HOST during the call; every pointer inside them is a DEVICE pointer.
 * Returns
 *   BT_EINVAL        a null pointer (x, x->data, blk, w1, b1, w2, b2, workspace, out); F, h, w, a channel count or `stride`
 *                    below 1; a negative stride of the view; w1, w2, wd or the workspace not 16-byte aligned; wd or bd present
 *                    when stride is 1, or absent when it is 2;
 *   BT_EUNSUPPORTED  c_in or c_out outside {64, 96, 128}; x->C != c_in; a stride above 2; stride 1 with c_in != c_out;
 *                    F above 65535; a size, a stride or an element offset of the view, or an element count (of x, or
 *                    maps * F * c_out * ho * wo with 2 maps at stride 1 and 3 at stride 2) above 2^31 - 1;
 *   BT_OK            otherwise;   BT_EHIP if a launch fails.
 * Every refusal happens before any HIP call. */
struct bt_res_block {            /* a tag only: the name without `struct` is the function's */
    const float *w1, *b1, *w2, *b2, *wd, *bd;
    int64_t c_in, c_out, stride;
};

size_t bt_res_block_workspace_bytes(int64_t F, int64_t c_out, int64_t h_in, int64_t w_in, int64_t stride);

int bt_res_block(const bt_encoder_level *x, const struct bt_res_block *blk, int64_t F, void *workspace, float *out, void *stream);

/* bt_encoder_stem — the stem (blocks.py: `relu1(norm1(conv1(x)))`, norm_fn = "instance").  Inference only, float32.
 * x is a strided view [F, BT_ENC_CIMG = 3, h, w] read in place; ho = (h - 1) / 2 + 1, wo likewise; out is a contiguous
 * [F, BT_ENC_CSTEM = 64, ho, wo] (possibly a slice of a larger buffer) that must NOT overlap x: the raw map is written into it
 * while other tiles still read x.  Any h, w >= 1.
 *
 *   raw = conv1(x) + bias:   7 x 7, stride 2, zero padding 3 OF THE IMAGE: output (y, x) has its centre tap at input
 *     (2 y, 2 x), a tap outside the h x w image contributing 0.  Summed on v_mfma_f32_16x16x4_f32 as float32 fma chains in
 *     one order for every pixel of every frame: kernel row ky ascending; within a row channel c ascending; within a channel
 *     kx ascending, 0..7, where kx = 7 is a zero weight times 0 or a finite image value (it leaves the chain's bits as they
 *     are).  The chain of a kernel row (21 products) starts from zero and is added into the total when the row ends: seven
 *     rounded adds, ky ascending; the bias is added last.
 *   statistics per (frame, channel) over the n = ho * wo pixels: as the head's and the trunk's (float64 sum and sum of
 *     squares of the stored float32 values, one partial per 16 x 8 tile, added in tile order; no floating-point atomics);
 *     mean = sum / n; var = max(sumsq / n - mean^2, 0); rstd = 1 / sqrt(var + 1e-5) in float64, stored as floats m, r.
 *   out = max(fl(fl(raw - m) * r), 0).  A constant channel has an exact mean, so it is exactly 0.
 *
 * `w_packed` is conv1.weight repacked as [7][3][8][64], 16-byte aligned: w_packed[ky][c][kx][m] = W[m][c][ky][kx] for
 * kx < 7, and w_packed[ky][c][7][m] = 0: the eighth entry MUST be zero.
 *
 * Three launches (convolution into out, statistics, normalisation of out in place), no host read.  The order of every sum is
 * fixed: a call repeats bit for bit, and frame f of F frames has the bits of that frame alone.
 *
 * workspace: bt_encoder_stem_workspace_bytes(F, h_in, w_in) bytes (0 when refused), 16-byte aligned: the tiles' partials and
 * the statistics, no map.  Every byte that is read is written first: it needs NO initialisation.
 * `x` is read on the HOST during the call; x->data and every other pointer is a DEVICE pointer.  The library allocates nothing.
 * Returns
 *   BT_EINVAL        a null pointer (x, x->data, w_packed, bias, workspace, out); F, h, w, x->C or c_out below 1; a negative
 *                    stride of the view; w_packed or the workspace not 16-byte aligned;
 *   BT_EUNSUPPORTED  x->C != 3 or c_out != 64; F above 65535; a size, a stride or an element offset of the view, the element
 *                    count F * 64 * ho * wo or the tile count above 2^31 - 1;
 *   BT_OK            otherwise;   BT_EHIP if a launch fails.
 * Every refusal happens before any HIP call. */
#define BT_ENC_CIMG 3
#define BT_ENC_CSTEM 64

size_t bt_encoder_stem_workspace_bytes(int64_t F, int64_t h_in, int64_t w_in);

int bt_encoder_stem(const bt_encoder_level *x, const float *w_packed, const float *bias, int64_t c_out, int64_t F, void *workspace,
                    float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_ENCODER_H */
