/* batrack_attn.h — C ABI of the attention core of the tracker's update transformers (the reference's
 * main/frontend/core/cotracker/blocks.py:280-305, `AttnBlock`, and :388-457, `UpdateFormer`; the attention itself is timm's
 * `Attention`): fused float32 attention over STRIDED sequences.  It reads q, k and v in place from the output of the qkv
 * Linear and writes the result in the layout the proj Linear wants; it forms no score matrix and makes no rearranged copy.
 * The row-wise parts of a block (LayerNorm, the four Linears, GELU) are torch operations: batrack_amd/frontend/update_former.py.
 *
 * Layout.  Token i (0 <= i < L) of sequence b (0 <= b < n_seq) is row r = b * seq_stride + i * tok_stride of both matrices.
 *   qkv   row r starts at qkv + r * qkv_row_stride; within it q of head h is at columns h * head_dim .. + head_dim - 1, k at
 *         heads * head_dim + h * head_dim, v at 2 * heads * head_dim + h * head_dim (timm: reshape(B, L, 3, heads, head_dim)).
 *   out   row r starts at out + r * out_row_stride; head h is at columns h * head_dim.
 * For the transformer's x [N, S, C] (B = 1; token (n, t) is row n * S + t, as in batrack_track.h):
 *   the time axis   n_seq = N, L = S, seq_stride = S, tok_stride = 1;
 *   the space axis  n_seq = S, L = N, seq_stride = 1, tok_stride = S.
 * Columns of a row past 3 * heads * head_dim (of out: past heads * head_dim) are neither read nor written; the same holds for
 * rows that no token addresses.  The sequences must not share rows (the caller's strides decide that; it is not checked).
 *
 * Arithmetic.  Per sequence and head, out_i = sum_j softmax_j((q_i . k_j) * scale) v_j, everything float32 on
 * v_mfma_f32_16x16x4_f32 (an exact float32 fma chain; there is no reduced-precision path).  The order is the kernel's own:
 *   logit     partial fma chains from 0 over the head columns d = 12 g + s, s outer, g = 0 .. 3 inner (the lane group g
 *             loads columns 12 g .. 12 g + 11 of its row as three float4).  Short path: four chains, chain c over
 *             s = 3 c .. 3 c + 2, added as (c0 + c1) + (c2 + c3).  Long path: two chains, s = 0 .. 5 and s = 6 .. 11, added
 *             (four would cost a wave per SIMD in registers).  A blocked sum: one chain of 48 roundings carries about
 *             1.5 x the error of the reference's GEMM.  Then ONE multiply by scale.
 *   short path, L <= BT_ATTN_SHORT_L (one wave per sequence and head, nothing staged in LDS):
 *             m_i = max_j logit; p_j = expf(logit_j - m_i); the denominator is ((p_{4g} + p_{4g+1}) + p_{4g+2}) + p_{4g+3}
 *             per g, then (g ^ 1) added, then (g ^ 2); the numerator two fma chains from 0 over j = 4 g + r (r = 0, 2 and r = 1, 3; r outer,
 *             g inner), added; out = numerator / denominator, one division.
 *   long path (a workgroup of 4 waves owns BT_ATTN_Q_TILE consecutive queries of one sequence and head, 32 a wave; keys
 *             and values pass through LDS in tiles of BT_ATTN_K_TILE, staged once per workgroup): the online softmax.  Per
 *             key tile: m' = max(m, max of the tile's logits), a = expf(m - m'), p_j = expf(logit_j - m'); each lane group g
 *             keeps its own partial denominator l_g = l_g * a + (sum of its 16 p of the tile, key 16 u + 4 g + r in the order
 *             u outer, r inner); the numerator is multiplied by a and continues its fma chain over the tile's keys in the
 *             order u = 0 .. 3 outer, r = 0 .. 3 middle, g = 0 .. 3 inner.  After the last tile the four l_g are added as on
 *             the short path and out = numerator / denominator.
 * The row maximum is subtracted before the exponential (expf, not an exp2 approximation): finite logits of any size give
 * finite output.  Keys >= L of a tile are masked to -inf, query rows >= L are not stored, and NO row >= L is loaded: it may
 * belong to another sequence or lie outside the buffer.
 * A non-finite value in a token's q reaches only that token's output row of that head; a non-finite value in k or v reaches
 * only its own sequence and head.  No workspace, no atomics: a call repeats bit for bit.
 * When qkv, out and both row strides are multiples of 16 bytes the rows are moved as float4, otherwise as scalars: the
 * same arithmetic in the same order.
 *
 * All pointers are DEVICE pointers; `stream` is a hipStream_t as void*.  Returns
 *   BT_EINVAL        a null qkv or out; n_seq < 0; L < 1; heads < 1; head_dim < 1; qkv_row_stride < 3 * heads * head_dim or
 *                    out_row_stride < heads * head_dim; seq_stride < 1 or tok_stride < 1; a non-finite scale;
 *   BT_EUNSUPPORTED  head_dim != BT_ATTN_HEAD_DIM; n_seq, seq_stride, tok_stride or a row stride above BT_ATTN_MAX_INDEX;
 *                    L above BT_ATTN_MAX_INDEX - BT_ATTN_Q_TILE (the tile loops count in int);
 *                    the largest row index (n_seq - 1) * seq_stride + (L - 1) * tok_stride above BT_ATTN_MAX_INDEX (so that
 *                    row index * row stride stays below 2^62); more than BT_ATTN_MAX_BLOCKS workgroups of 256 threads
 *                    (short: ceil(n_seq * heads / 4); long: n_seq * heads * ceil(L / BT_ATTN_Q_TILE)): a launch holds
 *                    fewer than 2^32 threads;
 *   BT_OK            otherwise — with nothing launched for n_seq == 0;   BT_EHIP if the launch fails.
 * Every refusal happens before anything is launched. */
#ifndef BATRACK_ATTN_H
#define BATRACK_ATTN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BT_ATTN_HEAD_DIM 48            /* the tracker's: hidden 384, 8 heads */
#define BT_ATTN_SHORT_L 16             /* up to here: one wave per (sequence, head) */
#define BT_ATTN_Q_TILE 128             /* long path: queries per workgroup */
#define BT_ATTN_K_TILE 64              /* long path: keys per LDS tile */
#define BT_ATTN_MAX_INDEX 2147483647LL /* 2^31 - 1 */
#define BT_ATTN_MAX_BLOCKS 16777215LL  /* 2^24 - 1 */

int bt_attention(const float *qkv, int64_t qkv_row_stride, float *out, int64_t out_row_stride,
                 int64_t n_seq, int64_t L, int64_t seq_stride, int64_t tok_stride,
                 int64_t heads, int64_t head_dim, float scale, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_ATTN_H */
