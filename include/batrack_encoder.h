/* batrack_encoder.h — C ABI of the feature encoder's head (the reference's main/frontend/core/cotracker/blocks.py:241-273,
 * the last third of `BasicEncoder.forward` with norm_fn = "instance" and shallow = False): the four pyramid levels resized
 * to the output map, their concatenation convolved 3 x 3 from 416 to 256 channels, the instance normalisation, the ReLU and
 * the 1 x 1 convolution to 128 channels.  Neither the resized copies nor the concatenation is ever in memory: the
 * convolution samples the four small maps while it stages its input.  conv1, norm1 and layer1..4 are not here.
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

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_ENCODER_H */
