/* batrack_rows.h — C ABI of the row-wise parts of the tracker's update transformers (the reference's
 * main/frontend/core/cotracker/blocks.py:280-305, `AttnBlock`: LayerNorm, the four Linears, GELU and the residual adds) as ONE
 * fused launch on the gfx950 f16 matrix pipe (v_mfma_f32_16x16x32_f16), at float32 accuracy by an operand split.  The opt-in
 * second route of batrack_amd/frontend/update_former.py (`rows_linear`, `attn_block_rows`, `forward_rows`); the attention core
 * between the Linears stays bt_attention (batrack_attn.h).
 *
 *   out[r, n] = residual[r, n] + act( (sum_k pro(x[r, :])[k] * W[n, k]) / s + bias[n] )        0 <= r < rows, 0 <= n < Nout
 *
 *   x         [rows, K] float32, row r at x + r * ldx (ldx >= K): a column slice of a wider matrix is read in place.
 *   w_hi/w_lo [Nout, K] f16, contiguous: the weight pre-split by update_former.pack_linear with the power of two s,
 *             hi = f16(W s), lo = f16(W s - float(hi)); inv_scale = 1 / s.
 *   bias      [Nout] float32 or NULL;  residual [rows, Nout] with row stride ldr, or NULL;  out [rows, Nout] with row stride ldo.
 *   prologue  BT_ROWS_PRO_NONE, or BT_ROWS_PRO_LAYERNORM: LayerNorm over the K columns without affine parameters, float32, two
 *             passes: mean = sum / K, var = sum((v - mean)^2) / K (biased), rstd = 1 / sqrt(var + eps), pro(v) = (v - mean) * rstd.
 *             Both sums are taken by 16 lanes: lane j adds the columns 4 c .. 4 c + 3 of the chunks c = j, j + 16, ... in
 *             ascending order into one chain from 0, then the 16 partial sums are added by a butterfly (xor 8, 4, 2, 1).
 *   act       BT_ROWS_ACT_NONE, or BT_ROWS_ACT_GELU_TANH: 0.5 v (1 + tanh(sqrt(2 / pi) (v + 0.044715 v^3))).
 *   precision BT_ROWS_F16X3: each activation a = pro(x) is split in the kernel as hi = f16(clamp(a, +-65504)) (round to nearest),
 *             lo = f16(clamp(a - float(hi), +-65504)), NaN passing through, and per K step of 32 three MFMAs are accumulated into
 *             ONE float32 accumulator in the order hi.hi, hi.lo (activation hi, weight lo), lo.hi.  Every f16 x f16 product is
 *             exact in float32; only lo.lo, of relative size 2^-22, is dropped.
 *             BT_ROWS_F16: the same code with the two cross products skipped: f16 accuracy (2^-11 per operand).
 *             The accumulated sum is multiplied by inv_scale (exact for a power of two) before the bias.
 *
 *             Where hi saturates (|a| > 65488, so hi = +-65504; 65488 itself is a tie and rounds to 65472) lo is as large as hi and lo.lo no longer negligible: for
 *             those activations alone a fourth product lo.lo is added after the three (every other activation enters it as an
 *             exact zero, and a workgroup skips it for a K step whose tile holds none: the result does not depend on the skip).
 *
 * Domain.  |pro(x)| <= 65488 keeps 22 significant bits.  From there to 131008 hi is +-65504 and lo = f16(a - hi) takes the rest
 * with f16's 11 bits: exact where a - hi has no more (1e5 is), within 16 in magnitude otherwise.  Beyond 131008 the result is
 * finite and WRONG, and an infinity in x gives a finite or a NaN result, never a trap.  Nothing in the update transformer
 * comes near it: LayerNorm output is bounded by sqrt(K), attention output by max |v|.  An activation below 2^-24 in
 * magnitude contributes nothing (f16 underflow); one below 2^-14 is held to 2^-24 absolute.
 *
 * The order of a row's arithmetic depends neither on where the row or the column lies in a tile nor on `rows`: the K steps
 * run from 0 in steps of 32 for every tile, the statistics of a row are taken by 16 lanes in the order above, and the
 * epilogue is one expression per element.  A row of a call on a slice of x equals that row of the full call bit for bit, and
 * a call repeats bit for bit (no atomics, no workspace).  A non-finite value in a row of x reaches that row of out only;
 * one in a row of W reaches that column of out only.  Row, column and K tails are zero-filled in LDS and never loaded: no
 * load or store addresses memory outside the tensors.
 * When x, w_hi, w_lo are 16-byte aligned and ldx is a multiple of 4 the operands are moved 16 bytes at a time, otherwise as
 * scalars: the same arithmetic in the same order.  out, residual and bias are addressed as scalars and need 4-byte alignment only.
 * out may BE residual (same pointer and row stride: each element is read and written by one lane).
 *
 * All pointers are DEVICE pointers; `stream` is a hipStream_t as void*.  Returns
 *   BT_EINVAL        a null x, w_hi, w_lo or out; rows < 0; Nout < 1; K < 8 or K % 8 != 0; ldx < K, ldo < Nout or (with a
 *                    residual) ldr < Nout; an unknown prologue, act or precision; a non-finite or non-positive inv_scale; with the
 *                    LayerNorm a negative or non-finite eps; out overlapping x; out overlapping residual other than being it;
 *   BT_EUNSUPPORTED  rows, K, Nout or a row stride above BT_ROWS_MAX_INDEX, or more than BT_ROWS_MAX_INDEX workgroups
 *                    (ceil(rows / BT_ROWS_TILE) * ceil(Nout / BT_ROWS_TILE));
 *   BT_OK            otherwise — with nothing launched for rows == 0;   BT_EHIP if the launch fails.
 * Every refusal happens before anything is launched. */
#ifndef BATRACK_ROWS_H
#define BATRACK_ROWS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BT_ROWS_TILE 128               /* output rows and columns per workgroup of 256 threads */
#define BT_ROWS_KSTEP 32               /* the K of one MFMA */
#define BT_ROWS_MAX_INDEX 2147483647LL /* 2^31 - 1 */

enum { BT_ROWS_PRO_NONE = 0, BT_ROWS_PRO_LAYERNORM = 1 };
enum { BT_ROWS_ACT_NONE = 0, BT_ROWS_ACT_GELU_TANH = 1 };
enum { BT_ROWS_F16X3 = 0, BT_ROWS_F16 = 1 };

int bt_rows_linear(const float *x, int64_t ldx, const void *w_hi, const void *w_lo, float inv_scale, const float *bias,
                   const float *residual, int64_t ldr, float *out, int64_t ldo,
                   int64_t rows, int64_t K, int64_t Nout, int prologue, float eps, int act, int precision, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_ROWS_H */
