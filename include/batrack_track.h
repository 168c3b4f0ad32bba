/* batrack_track.h — C ABI of the tracker's refinement iteration around its two update transformers
 * (the reference's main/frontend/md_tracker.py:181-413, `MDTracker.forward_iteration`, and :49-61, `sample_pos_embed`):
 * the position embedding of the tracks, the transformer's input tokens in one launch, and the state update from the
 * transformer's output in one launch.  The transformers themselves are not here: their attention core is batrack_attn.h.
 *
 * Layouts.  B = 1.  State tensors are frame-major, as the correlation lookup (batrack_corr.h) wants them:
 * coords [S, N, 3] (x, y, z), ffeats [S, N, C], track_mask [S, N], vis [S, N], fcorrs [S, N, LRR], float32 contiguous.
 * Tokens and deltas are token-major: x [N, S, E], delta [N, S, 3 + C]; token (n, t) is row n * S + t.  The kernels do the
 * (s, n) <-> (n, s) row transposition.
 *
 * bt_track_pos_embed.  The 2-D sin-cos table T[y, x, :] = [tabx[x, :] | taby[y, :]] (tabx [W, E/2], taby [H, E/2]; the
 * table is separable and is never formed) sampled bilinearly at the N points (x, y) = coords[k * coord_stride + 0 .. 1]
 * (frame 0 of the window: what the reference passes), as bilinear_sample2d does (frontend/core/model_utils.py:75-158):
 *   x0 = floor(x), x1 = x0 + 1 (the same for y); the four corner indices clamped to the map; the weights from the UNCLAMPED
 *   corners, (x1 - x)(y1 - y), (x - x0)(y1 - y), (x1 - x)(y - y0), (x - x0)(y - y0); every product rounded, the four
 *   products summed left to right.  out [N, E].  Bit-equal to the reference's float32 run given tables that are the
 *   float32 rounding of its float64 table — for EVERY finite coordinate, the reference run on an x86 host: it takes x0 as
 *   floor(x).int(), and a floor that does not fit an int32 (|x| >= 2^31 on either side) becomes INT_MIN there, as it does
 *   here.  What then holds for finite coordinates (tests/golden/pos_embed_far.npz records it):
 *     both coordinates below 2^31 in size   the sample; from 2^24 up x0 = x, x1 = x0 + 1 rounds to even, the weights are 0, 1 or 2;
 *     one coordinate beyond                 its two weights are +-(x + 2^31), the clamped indices coincide at 0 and the four
 *                                           terms cancel up to their rounding: zero, or a finite residue of the size of an
 *                                           ulp of the weight when the other coordinate has a fractional part;
 *     both beyond (or one beyond, the other from 2^24 + 2 up) with |x - x0| |y - y0| above FLT_MAX   NaN (inf - inf).
 *   A NaN or infinite coordinate gives non-finite values; whatever a coordinate is, it touches its own row only.
 *
 * bt_track_tokens.  x [N, S, E], E = F + LRR + C + 2.  With c = coords - coords_sub (coords_sub may be null: c = coords)
 * and flow[n, t, :] = c[t, n, :] - c[0, n, :]:
 *   columns 0 : F        W_flow . emb + b_flow, emb [195] = [pe_x | pe_y | pe_z | flow], pe_v[2k] = sin(v d_k),
 *                        pe_v[2k+1] = cos(v d_k), d_k = 2k * 15.625 (k = 0 .. 31), the product v d_k ONE float32 multiply,
 *                        sine and cosine with full argument reduction (arguments reach 1e5 rad).  W_flow [F, 195] and
 *                        b_flow [F] as nn.Linear stores them.  Summed on v_mfma_f32_16x16x4_f32: a float32 fma chain over
 *                        the 195 inputs in the kernel's own order (csrc/track_iter.hip), then + b_flow.
 *   columns F : F+LRR    fcorrs[t, n, :]
 *   the next C           ffeats[t, n, :]
 *   the last 2           fix_track_mask != 0: (track_mask[t, n], vis[t, n]).
 *                        fix_track_mask == 0: the reference concatenates the two along N and then reshapes
 *                        (md_tracker.py:281-285): slot c of token (n, t) is element f = n * 2S + 2t + c of the
 *                        [2N, S] array [track_mask^T ; vis^T]: m = f / S, s = f % S, track_mask[s, m] if m < N, else
 *                        vis[s, m - N].
 *   then every column:   x = (value + pos[n, col]) + time[t, col], in that order (pos [N, E], time [S, E]).
 * The copy columns (F and up) are bit-equal to the reference's float32 run.  A NaN or infinite coordinate makes the flow
 * columns of the tokens whose flow it enters non-finite (frame t > 0: token (n, t) alone; frame 0: the S tokens of track n)
 * and touches no other token.
 *
 * bt_track_apply.  From delta [N, S, 3 + C], in place:
 *   state[t, n, :] += delta[n, t, 0:3]                                   one float32 add: bit-equal to the reference
 *   ffeats[t, n, :] += GELU_erf(W_u . GN(delta[n, t, 3:]) + b_u)         GN: (v - mean) / sqrt(var + 1e-5) * gamma + beta
 *                                                                        over the row's C channels, biased variance;
 *                                                                        W_u [C, C], gamma, beta, b_u [C]; the moments,
 *                                                                        the normalisation and the C-term sums in
 *                                                                        double (v_mfma_f64_16x16x4_f64), erff and the
 *                                                                        last add in float32
 *   out[t, n, 0:2] = p[0:2] * stride;  out[t, n, 2] = (p[2] / Dz) * d_range + d_near, through exp when use_log_depth,
 *                                                                        every operation rounded (d_range = d_far - d_near)
 *   total == null:   p = state (the tracker's `coords`).
 *   total != null:   the static pass (md_tracker.py:400-411): state is `coords_dyn`, dyn_mask [N] the motion label after
 *                    its sigmoid, p = total[t, n, :] - state[t, n, :] * dyn_mask[n].
 *
 * No workspace, no atomics: a call repeats bit for bit.  All pointers are DEVICE pointers; `stream` is a hipStream_t as
 * void*.  Returns
 *   BT_EINVAL        a null pointer (coords_sub and total may be null; dyn_mask only when total is), a non-positive S, a
 *                    negative N, H, W < 1, E < 2 or odd, coord_stride < 2, F, LRR < 1, C < 1, C % 16 != 0 (apply);
 *   BT_EUNSUPPORTED  F > BT_TRACK_MAX_F (the weight fragments of 9 column tiles of 16 fill the LDS), C > BT_TRACK_MAX_C
 *                    (apply: W_u and the waves' delta tiles fill the LDS), LRR or C (tokens) or E above 65536, H or W
 *                    above 32768, S * N above 2^31 - 17;
 *   BT_OK            otherwise — with nothing launched for N == 0;   BT_EHIP if a launch fails.
 * Every refusal happens before anything is launched. */
#ifndef BATRACK_TRACK_H
#define BATRACK_TRACK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BT_TRACK_EMB 195      /* 3 * 64 sin-cos entries and the flow itself */
#define BT_TRACK_MAX_F 144
#define BT_TRACK_MAX_C 128

int bt_track_pos_embed(const float *tabx, const float *taby, int64_t H, int64_t W, int64_t E,
                       const float *coords, int64_t coord_stride, int64_t N, float *out, void *stream);

int bt_track_tokens(const float *coords, const float *coords_sub, const float *fcorrs, const float *ffeats,
                    const float *track_mask, const float *vis, const float *pos, const float *time,
                    const float *w_flow, const float *b_flow, int64_t S, int64_t N, int64_t F, int64_t LRR, int64_t C,
                    int32_t fix_track_mask, float *x, void *stream);

int bt_track_apply(const float *delta, const float *gamma, const float *beta, const float *w_u, const float *b_u,
                   float *state, float *ffeats, const float *total, const float *dyn_mask,
                   int64_t S, int64_t N, int64_t C, float stride, float Dz, float d_range, float d_near,
                   int32_t use_log_depth, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BATRACK_TRACK_H */
