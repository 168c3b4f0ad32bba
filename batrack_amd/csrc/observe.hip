// observe.hip — the step between the tracker's forward pass and the bundle adjustment fused for gfx950: the new edges'
// targets and weights, the motion-decoupled pose weights, the keyframes' `patches_valid_` rows, the queries' mono
// disparity and the scatter into the tracks' window buffers (specification: include/batrack_observe.h,
// bt_observe_window).  Formulas: the reference's main/batrack.py:575-587 (tracker tail), :667-757 (get_window_trajs),
// :760-818 (predict_target), :632-663 (update_local), frontend/core/model_utils.py:75-158 (bilinear_sample2d).
//
// Three launches of fixed shape:
//   k_observe_query      a lane per query: the bilinear sample of its frame's depth map -> query_disp.
//   k_observe_threshold  ONE workgroup: the two order statistics floor / ceil of the quantile's rank over all S*Nq static
//                        scores by the 8-bit radix select of radix_select.hpp (four passes for the lower one, a fifth — the
//                        smallest key above it — only when the upper one is another value), torch.lerp's fused form, the
//                        min with STATIC_THRESHOLD.  The threshold is left in the workspace: no host round trip.
//   k_observe_window     a workgroup per OB_TRACKS consecutive queries.  The inputs are frame-major, the outputs
//                        track-major: phase A reads each frame's row for the block's tracks coalesced (lanes over tracks)
//                        and keeps (x, y, disparity, labels) of the (track, s) tile in LDS; a lane per track then takes the
//                        two counts and settles patches_valid; phase B walks the flattened (track, s) index, so that the
//                        block's S'*OB_TRACKS edges are written as contiguous runs (12-byte records as in k_world_tracks).
// No atomics on floats, no scratch: a call repeats bit for bit.  Everything here rounds every operation (contraction
// off) and divides with the correctly rounded division: the file must not be built with a fast-math flag.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_observe.h"
#include "radix_select.hpp"
#include "sample_taps.hpp"

#pragma clang fp contract(off)

namespace bt {

constexpr int OB_TRACKS = 32;                   // queries of one workgroup of the window pass
constexpr int OB_THREADS = 256;
constexpr int OB_LD = OB_TRACKS + 1;            // LDS row stride of the (s, track) tile: both phases conflict-free
constexpr int OB_SEL_THREADS = 1024;            // the threshold's single workgroup

struct OF3 { float x, y, z; };                  // 12-byte record, 4-byte aligned
struct OF2 { float a, b; };

struct ObQuery {                              // the scalars of the query pass
    const float *queries, *dmaps;
    float *query_disp;
    int Nq, Sp, H, W;
};

__global__ __launch_bounds__(256) void k_observe_query(ObQuery a) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.Nq) return;
    const float tf = a.queries[3 * q], x = a.queries[3 * q + 1], y = a.queries[3 * q + 2];
    float d = NAN;
    if (tf >= 0.0f && tf < (float)a.Sp) {
        const int t = (int)tf;
        d = bilinear_clamped(a.dmaps + (size_t)t * a.H * a.W, a.H, a.W, x, y);
    }
    a.query_disp[q] = 1.0f / clamp_min_1e2(d);
}

// static = 1 - dyn over n values; a = the k0-th, b = the k1-th smallest (k1 = k0 or k0 + 1); *th = min(lerp(a, b, w), st)
__global__ __launch_bounds__(OB_SEL_THREADS) void k_observe_threshold(const float *__restrict__ dyn, int n, int k0, int k1,
                                                                       float w, float st, float *__restrict__ th) {
    __shared__ uint32_t h[rs::kBins];
    __shared__ uint32_t s_prefix, s_rank, s_cnt, s_nan;
    __shared__ uint32_t s_min[OB_SEL_THREADS / 64];
    const int tid = threadIdx.x;
    uint32_t prefix = 0, rank = (uint32_t)k0;
    if (tid == 0) s_nan = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t mask = rs::fixed_mask<uint32_t>(pass, shift);
        if (tid < rs::kBins) h[tid] = 0;
        __syncthreads();
        for (int base = 0; base < n; base += OB_SEL_THREADS) {                 // every lane of a wave walks the loop
            const int i = base + tid;
            bool act = i < n;
            uint32_t key = 0;
            if (act) {
                const float v = dyn[i];
                if (pass == 0 && v != v) s_nan = 1;
                key = rs::fkey(1.0f - v);
                act = rs::carries(key, prefix, mask);
            }
            rs::hist_add(h, key, shift, act);
        }
        __syncthreads();
        if (tid < 64) {                                                        // one wave: the bin that holds `rank`
            uint32_t c[4], excl, inc, total;
            rs::wave_scan(h, c, excl, inc, total);
            if (excl <= rank && rank < inc) {
                uint32_t rem, cnt;
                const int d = rs::find_digit(c, excl, rank, rem, cnt);
                s_prefix = prefix | ((uint32_t)d << shift);
                s_rank = rem;
                s_cnt = cnt;
            }
        }
        __syncthreads();
        prefix = s_prefix;
        rank = s_rank;
    }
    const uint32_t cnt = s_cnt;                                                // values equal to the k0-th; rank < cnt
    uint32_t key1 = prefix;
    if (k1 != k0 && rank + 1 >= cnt) {                                         // the next one is another value: the smallest key above
        uint32_t m = 0xffffffffu;
        for (int i = tid; i < n; i += OB_SEL_THREADS) {
            const uint32_t key = rs::fkey(1.0f - dyn[i]);
            if (key > prefix && key < m) m = key;
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t o = __shfl_xor(m, d);
            m = o < m ? o : m;
        }
        if ((tid & 63) == 0) s_min[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) {
            for (int i = 1; i < OB_SEL_THREADS / 64; ++i) m = s_min[i] < m ? s_min[i] : m;
            key1 = m;
        }
    }
    if (tid == 0) {
        const float a = rs::fdecode(prefix), b = rs::fdecode(key1), diff = b - a;
        float q = w < 0.5f ? fmaf(w, diff, a) : fmaf(w - 1.0f, diff, b);       // torch.lerp on the CPU, fused
        if (s_nan) q = NAN;
        *th = st < q ? st : q;                                                 // Python's min(q, st): a NaN q stays
    }
}

struct ObWindow {                               // the scalars of the window pass
    const float *traj, *depth, *vis, *dyn, *queries, *th;
    const int64_t *ii, *jj, *kk;
    float *patches_valid, *patches_local, *l_mono, *l_vis, *l_static, *l_weights, *targets, *weights, *weights_pose;
    int64_t Nq, NM, lo, M, kf_stride, n, min_track_len;
    int Sp, S_local, mid, tail, has_vt, is_init;
    float sx, sy, rx, ry, vt, lo_x, hi_x, lo_y, hi_y;
};

__global__ __launch_bounds__(OB_THREADS) void k_observe_window(ObWindow a) {
    extern __shared__ float s_tile[];                            // S' * OB_LD entries each: x, y, disparity, labels (13 B an entry)
    __shared__ int s_keep[OB_TRACKS];
    const int tid = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * OB_TRACKS;
    const int nt = (int)(a.Nq - q0 < OB_TRACKS ? a.Nq - q0 : OB_TRACKS);
    const int Sp = a.Sp;
    float *s_x = s_tile, *s_y = s_x + Sp * OB_LD, *s_z = s_y + Sp * OB_LD;
    unsigned char *s_f = reinterpret_cast<unsigned char *>(s_z + Sp * OB_LD);    // bit 0 vis_label, 1 vis_raw, 2 static_label
    // ---- phase A: lanes over tracks, eight frames at a time
    {
        const int t = tid & (OB_TRACKS - 1);
        if (t < nt) {
            const int64_t q = q0 + t;
            const float th = *a.th;
            int tq = -1;
            float qx = 0.0f, qy = 0.0f;
            if (a.tail) {
                const float tf = a.queries[3 * q];
                if (tf >= 0.0f && tf < (float)Sp) tq = (int)tf;
                qx = a.queries[3 * q + 1] * a.sx;                                // batrack.py:547-548
                qy = a.queries[3 * q + 2] * a.sy;
            }
            for (int s = tid / OB_TRACKS; s < Sp; s += OB_THREADS / OB_TRACKS) {
                const int64_t idx = (int64_t)s * a.Nq + q;
                float x = a.traj[2 * idx], y = a.traj[2 * idx + 1], v = a.vis[idx];
                if (a.tail) {
                    if (s == tq) { x = qx; y = qy; v = 1.0f; }                   // :580-582
                    x *= a.rx;                                                   // :584-585
                    y *= a.ry;
                }
                const float z = 1.0f / clamp_min_1e2(a.depth[idx]);               // :765
                const float stat = 1.0f - a.dyn[idx];                            // :718
                const bool vl = a.has_vt ? v > a.vt : true;                      // :707-710
                const bool in = x >= a.lo_x && x < a.hi_x && y >= a.lo_y && y < a.hi_y;   // :713
                const int o = s * OB_LD + t;
                s_x[o] = x; s_y[o] = y; s_z[o] = z;
                s_f[o] = (unsigned char)((vl ? 1 : 0) | (vl && in ? 2 : 0) | (stat >= th ? 4 : 0));
            }
        }
    }
    __syncthreads();
    // ---- per track: the two counts, patches_valid
    if (tid < nt) {
        int nl = 0, nr = 0;
        for (int s = 0; s < Sp; ++s) {
            const int f = s_f[s * OB_LD + tid];
            nl += f & 1;
            nr += (f >> 1) & 1;
        }
        const int64_t q = q0 + tid;
        float *pvp = a.patches_valid + (a.lo + a.kf_stride * (q / a.M)) * a.M + q % a.M;
        bool keep = true, pv = false, write = false;
        if (a.is_init) { pv = *pvp != 0.0f || nl > 3; write = true; }            // :738-742
        if (a.n >= a.min_track_len) { keep = nr >= a.min_track_len; pv = keep; write = true; }   // :779-786
        if (write) *pvp = pv ? 1.0f : 0.0f;
        s_keep[tid] = keep;
    }
    __syncthreads();
    // ---- phase B: the block's edges, track-major
    const unsigned tot = (unsigned)nt * (unsigned)Sp;
    for (unsigned f = tid; f < tot; f += OB_THREADS) {
        const unsigned t = f / (unsigned)Sp;
        const int s = (int)(f - t * (unsigned)Sp);
        const int o = s * OB_LD + (int)t;
        const int fl = s_f[o];
        const OF3 tg = {s_x[o], s_y[o], s_z[o]};
        const float vr = (fl & 2) ? 1.0f : 0.0f, sl = (fl & 4) ? 1.0f : 0.0f;
        const float w = ((fl & 2) && s_keep[t]) ? 1.0f : 0.0f;
        const float wp = (fl & 4) ? w : 0.0f;                                    // :789-792
        const int64_t e = q0 * Sp + f;
        *reinterpret_cast<OF3 *>(a.targets + 3 * e) = tg;
        *reinterpret_cast<OF2 *>(a.weights + 2 * e) = OF2{w, w};
        *reinterpret_cast<OF2 *>(a.weights_pose + 2 * e) = OF2{wp, wp};
        const int64_t k = a.kk[e], slot = a.jj[e] - a.ii[e] + a.mid;             // :646-648
        if (slot >= 0 && slot < a.S_local && k >= 0 && k < a.NM) {
            const int64_t c = k * a.S_local + slot;
            *reinterpret_cast<OF3 *>(a.patches_local + 3 * c) = tg;
            if (a.l_mono) a.l_mono[c] = tg.z;
            if (a.l_vis) a.l_vis[c] = vr;
            if (a.l_static) a.l_static[c] = sl;
            if (a.l_weights) a.l_weights[c] = w;
        }
    }
}

}  // namespace bt

extern "C" size_t bt_observe_workspace_bytes(void) { return 64; }                // the threshold, one cache line of its own

extern "C" int bt_observe_window(const bt_observe_args *p, void *workspace, void *stream) {
    if (!p || !workspace) return BT_EINVAL;
    const bt_observe_args &a = *p;
    if (a.S < 1 || a.Sp < 0 || a.Sp > a.S || a.Nq < 0 || a.M < 1 || a.kf_stride < 1 || a.N < 1 || a.S_local < 1) return BT_EINVAL;
    if (a.Nq != (a.Sp + a.kf_stride - 1) / a.kf_stride * a.M || a.E != a.Nq * a.Sp) return BT_EINVAL;
    if (a.n < a.Sp || a.n > a.N || a.H < 1 || a.W < 1 || a.padding < 0) return BT_EINVAL;
    if (a.interp_w < 0 || a.interp_h < 0 || (a.interp_w == 0) != (a.interp_h == 0)) return BT_EINVAL;
    if (!(a.static_quantile >= 0.0 && a.static_quantile <= 1.0)) return BT_EINVAL;
    if (a.S > BT_OBSERVE_MAX_S || a.Nq >= (int64_t)1 << 24 || a.S * a.Nq >= (int64_t)1 << 24 || a.N > ((int64_t)1 << 31) / a.M ||
        a.S_local >= (int64_t)1 << 31 || a.N * a.M >= ((int64_t)1 << 31) / a.S_local || a.H >= ((int64_t)1 << 31) / a.W)
        return BT_EUNSUPPORTED;
    if (a.E == 0) return BT_OK;                   // nothing to read or write: the pointers are not looked at
    if (!a.traj || !a.depth || !a.vis || !a.dyn || !a.queries || !a.ii || !a.jj || !a.kk || !a.patches_valid || !a.patches_local ||
        !a.targets_3d || !a.weights || !a.weights_pose || (a.dmaps && !a.query_disp)) return BT_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *th = static_cast<float *>(workspace);
    if (a.dmaps) {
        bt::ObQuery q{a.queries, a.dmaps, a.query_disp, (int)a.Nq, (int)a.Sp, (int)a.H, (int)a.W};
        hipLaunchKernelGGL(bt::k_observe_query, dim3((unsigned)((a.Nq + 255) / 256)), dim3(256), 0, st, q);
    }
    {   // torch.quantile: the rank in float32, q = f32(1 - STATIC_QUANTILE)
        const int64_t nn = a.S * a.Nq;
        const float qf = (float)(1.0 - a.static_quantile), rank = qf * (float)(nn - 1);
        const float below = floorf(rank);
        hipLaunchKernelGGL(bt::k_observe_threshold, dim3(1), dim3(bt::OB_SEL_THREADS), 0, st, a.dyn, (int)nn, (int)below,
                           (int)ceilf(rank), rank - below, (float)a.static_threshold, th);
    }
    bt::ObWindow w{};
    w.traj = a.traj; w.depth = a.depth; w.vis = a.vis; w.dyn = a.dyn; w.queries = a.queries; w.th = th;
    w.ii = a.ii; w.jj = a.jj; w.kk = a.kk;
    w.patches_valid = a.patches_valid; w.patches_local = a.patches_local; w.l_mono = a.local_monodisp; w.l_vis = a.local_vis;
    w.l_static = a.local_static; w.l_weights = a.local_weights;
    w.targets = a.targets_3d; w.weights = a.weights; w.weights_pose = a.weights_pose;
    w.Nq = a.Nq; w.NM = a.N * a.M; w.lo = a.n - a.Sp; w.M = a.M; w.kf_stride = a.kf_stride; w.n = a.n; w.min_track_len = a.min_track_len;
    w.Sp = (int)a.Sp; w.S_local = (int)a.S_local; w.mid = (int)((a.S_local + 1) / 2 - 1);
    w.tail = a.interp_w > 0; w.has_vt = a.has_vis_threshold != 0; w.is_init = a.is_initialized != 0;
    if (w.tail) {                                   // the quotients in double, as Python takes them; rounded once
        w.sx = (float)((double)a.interp_w / (double)a.W); w.sy = (float)((double)a.interp_h / (double)a.H);
        w.rx = (float)((double)a.W / (double)a.interp_w); w.ry = (float)((double)a.H / (double)a.interp_h);
    }
    w.vt = (float)a.vis_threshold;
    w.lo_x = w.lo_y = (float)a.padding;
    w.hi_x = (float)(a.wd - (double)a.padding); w.hi_y = (float)(a.ht - (double)a.padding);
    hipLaunchKernelGGL(bt::k_observe_window, dim3((unsigned)((a.Nq + bt::OB_TRACKS - 1) / bt::OB_TRACKS)), dim3(bt::OB_THREADS),
                       (unsigned)(a.Sp * bt::OB_LD * 13), st, w);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
