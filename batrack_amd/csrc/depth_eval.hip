// depth_eval.hip — the video-depth metrics of the reference's compute_errors / eval_depth_metric (include/batrack_depth.h), gfx950.
//   k_de_hist     one histogram pass of the radix select of radix_select.hpp (4 passes) over the order-preserving uint32 keys of
//                 the valid gt and pred values, for four selections at once: the lower and upper middle element of each.
//   k_de_pick     its pick, one workgroup, one wave per selection; after the last pass the medians and their ratio (numpy's
//                 median: an even count takes the float64 mean of the two middle elements).
//   k_de_sums     least-squares scaling: per-workgroup count, means and centred second moments of (p, g) in float64, each thread's
//                 sums taken about its first valid element and merged pairwise (Chan et al.) in a fixed order;  k_de_solve: the
//                 same merge over the workgroups, s = Cpg / Cpp, t = mean g - s mean p, the rank decision from det = n Cpp
//                 (minimum-norm solution when singular, as np.linalg.lstsq).
//   k_de_metrics  scaling, clamping and the eight metrics' per-element terms in float64; per-workgroup float64 partials;
//   k_de_final    their fixed-order total.  No float atomics anywhere: a call is bit-for-bit repeatable.
// Workgroups hand results to each other only at kernel boundaries; everything is enqueued on the caller's stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_depth.h"
#include "radix_select.hpp"

namespace bt {
namespace de {

constexpr int kSel = 4;                          // gt lower, gt upper, pred lower, pred upper middle element
constexpr int kBins = rs::kBins;
constexpr int kPasses = 4;                       // 8-bit digits
constexpr int kHistThreads = 512, kHistBlocks = 512;
constexpr int kSumThreads = 256, kSumBlocks = 2048;
constexpr int kParts = 9;                        // abs_rel, sq_rel, log10, sq, sq_log, a1, a2, a3, count

struct State {
    uint32_t prefix[kSel];                       // key bits fixed so far
    uint32_t rank[kSel];                         // rank still to find among the keys that carry the prefix
    uint32_t count, nan_pred, pad[6];
    double scale, shift;                         // ratio or s; t
};

// workspace: histograms [kPasses][kSel][kBins] uint32 | State (256 B) | partials [kSumBlocks][kParts] float64
constexpr size_t kHistBytes = (size_t)kPasses * kSel * kBins * sizeof(uint32_t);
constexpr size_t kStateOff = kHistBytes, kPartOff = kHistBytes + 256;
constexpr size_t kWsBytes = kPartOff + (size_t)kSumBlocks * kParts * sizeof(double);
static_assert(sizeof(State) <= 256, "State");

using rs::fdecode;
using rs::fkey;

__device__ __forceinline__ State *state(unsigned char *ws) { return reinterpret_cast<State *>(ws + kStateOff); }
__device__ __forceinline__ double *partials(unsigned char *ws) { return reinterpret_cast<double *>(ws + kPartOff); }

// f(g, p, m) for every element of this thread's grid-stride share; 16-byte loads of gt and pred (4-byte of the mask) when VEC
template <bool VEC, class F>
__device__ __forceinline__ void for_elems(const float *gt, const float *pred, const uint8_t *mask, int64_t n, F &&f) {
    const int64_t nth = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t start = 0;
    if (VEC) {
        const int64_t n4 = n >> 2;
        for (int64_t i = tid; i < n4; i += nth) {
            const float4 g = reinterpret_cast<const float4 *>(gt)[i], p = reinterpret_cast<const float4 *>(pred)[i];
            const uint32_t m = mask ? reinterpret_cast<const uint32_t *>(mask)[i] : 0x01010101u;
            f(g.x, p.x, (m & 0xffu) != 0);
            f(g.y, p.y, (m & 0xff00u) != 0);
            f(g.z, p.z, (m & 0xff0000u) != 0);
            f(g.w, p.w, (m & 0xff000000u) != 0);
        }
        start = 4 * n4;
    }
    for (int64_t i = start + tid; i < n; i += nth) f(gt[i], pred[i], mask ? mask[i] != 0 : true);
}

template <bool VEC>
__global__ __launch_bounds__(kHistThreads) void k_de_hist(const float *gt, const float *pred, const uint8_t *mask, int64_t n, float dmin,
                                                          float dmax, unsigned char *ws, int pass) {
    __shared__ uint32_t h[kSel * kBins];
    __shared__ uint32_t s_nan;
    rs::hist_clear(h, kSel * kBins);
    if (threadIdx.x == 0) s_nan = 0u;
    __syncthreads();
    const State *st = state(ws);
    const int shift = 24 - 8 * pass;
    const uint32_t hi = rs::fixed_mask<uint32_t>(pass, shift);
    const uint32_t p0 = st->prefix[0], p1 = st->prefix[1], p2 = st->prefix[2], p3 = st->prefix[3];
    for_elems<VEC>(gt, pred, mask, n, [&](float g, float p, bool m) {
        const bool v = m && g > dmin && g < dmax;
        rs::add_pair(h, fkey(g), shift, hi, p0, p1, v);
        rs::add_pair(h + 2 * kBins, fkey(p), shift, hi, p2, p3, v);
        if (pass == 0) {
            const uint64_t b = __ballot(v && p != p);
            if (b && (int)__lane_id() == __ffsll((unsigned long long)b) - 1) atomicAdd(&s_nan, (uint32_t)__popcll(b));
        }
    });
    __syncthreads();
    rs::hist_flush(h, reinterpret_cast<uint32_t *>(ws) + (size_t)pass * kSel * kBins, kSel * kBins);
    if (pass == 0 && threadIdx.x == 0 && s_nan) atomicAdd(&state(ws)->nan_pred, s_nan);
}

__global__ __launch_bounds__(256) void k_de_pick(unsigned char *ws, int pass) {
    __shared__ uint32_t old[kSel];
    State *st = state(ws);
    const int w = threadIdx.x >> 6;
    if (threadIdx.x < kSel) old[threadIdx.x] = st->prefix[threadIdx.x];  // as the histogram pass saw them
    __syncthreads();
    const uint32_t *hh = reinterpret_cast<const uint32_t *>(ws) + ((size_t)pass * kSel + rs::shared_source(w, old)) * kBins;
    // pass 0: every valid element is counted in every selection's histogram; the middle ranks of the valid count
    const uint32_t total = rs::narrow(hh, [&](uint32_t t) { return pass == 0 ? rs::middle_rank(t, w & 1) : st->rank[w]; },
                                      24 - 8 * pass, st->prefix[w], st->rank[w]);
    if (pass == 0 && threadIdx.x == 0) st->count = total;
    if (pass == kPasses - 1) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t cnt = st->count;
            const double nan = __builtin_nan("");
            double mg = nan, mp = nan;
            if (cnt > 0) {
                const double gl = fdecode(st->prefix[0]), gu = fdecode(st->prefix[1]), pl = fdecode(st->prefix[2]), pu = fdecode(st->prefix[3]);
                mg = (cnt & 1u) ? gl : (gl + gu) / 2.0;
                mp = (cnt & 1u) ? pl : (pl + pu) / 2.0;
                if (st->nan_pred) mp = nan;                                 // np.median of an array with a NaN
            }
            st->scale = mg / mp;
        }
    }
}

__device__ __forceinline__ double block_sum_d(double v, double *red) {     // blockDim.x <= 1024; fixed order
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x < 64) {
        t = (int)threadIdx.x < nw ? red[threadIdx.x] : 0.0;
        for (int o = 8; o > 0; o >>= 1) t += __shfl_xor(t, o);
    }
    return t;                                                              // valid in thread 0
}

// least-squares scaling: count, means and centred second moments of the valid (p, g).  The raw sums of p^2 and p g would leave
// det = Spp n - Sp^2 to cancel on a pred of small relative spread; these do not.
struct Mom {
    double n, mp, mg, cpp, cpg;                  // count, mean p, mean g, sum (p - mp)^2, sum (p - mp)(g - mg)
};

// a then b as one set (Chan, Golub, LeVeque); an empty side leaves the other as it is
__device__ __forceinline__ Mom merge(const Mom &a, const Mom &b) {
#pragma clang fp contract(off)
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    Mom r;
    r.n = a.n + b.n;
    const double w = b.n / r.n, aw = a.n * w, dp = b.mp - a.mp, dg = b.mg - a.mg;
    r.mp = a.mp + dp * w;
    r.mg = a.mg + dg * w;
    r.cpp = a.cpp + b.cpp + dp * dp * aw;
    r.cpg = a.cpg + b.cpg + dp * dg * aw;
    return r;
}

__device__ __forceinline__ Mom block_merge(Mom v, Mom *red) {             // blockDim.x <= 1024; fixed order, the lower lane first
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        Mom u;
        u.n = __shfl_xor(v.n, o); u.mp = __shfl_xor(v.mp, o); u.mg = __shfl_xor(v.mg, o);
        u.cpp = __shfl_xor(v.cpp, o); u.cpg = __shfl_xor(v.cpg, o);
        v = (lane & o) ? merge(u, v) : merge(v, u);
    }
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < nw; ++i) v = merge(v, red[i]);
    return v;                                                              // valid in thread 0
}

template <bool VEC>
__global__ __launch_bounds__(kSumThreads) void k_de_sums(const float *gt, const float *pred, const uint8_t *mask, int64_t n, float dmin,
                                                         float dmax, unsigned char *ws) {
#pragma clang fp contract(off)
    __shared__ Mom red[16];
    // per thread: sums about its first valid element (p0, g0), which lies within the data's spread of their mean
    double c = 0.0, p0 = 0.0, g0 = 0.0, s1 = 0.0, s2 = 0.0, sg = 0.0, spg = 0.0;
    for_elems<VEC>(gt, pred, mask, n, [&](float g, float p, bool m) {
        if (m && g > dmin && g < dmax) {
            if (c == 0.0) { p0 = p; g0 = g; }
            const double dp = (double)p - p0, dg = (double)g - g0;
            c += 1.0; s1 += dp; s2 += dp * dp; sg += dg; spg += dp * dg;
        }
    });
    Mom v = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (c > 0.0) {
        v.n = c;
        v.mp = p0 + s1 / c;
        v.mg = g0 + sg / c;
        v.cpp = s2 - s1 * s1 / c;
        v.cpg = spg - s1 * sg / c;
    }
    v = block_merge(v, red);
    if (threadIdx.x == 0) {
        double *out = partials(ws) + (size_t)blockIdx.x * kParts;
        out[0] = v.n; out[1] = v.mp; out[2] = v.mg; out[3] = v.cpp; out[4] = v.cpg;
    }
}

__global__ __launch_bounds__(256) void k_de_solve(unsigned char *ws, int nb) {
#pragma clang fp contract(off)
    __shared__ Mom red[16];
    const double *part = partials(ws);
    Mom v = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nb; b += blockDim.x) {
        const double *q = part + (size_t)b * kParts;
        v = merge(v, Mom{q[0], q[1], q[2], q[3], q[4]});
    }
    v = block_merge(v, red);
    if (threadIdx.x != 0) return;
    // A = [p, 1]:  A^T A = [[Spp, Sp], [Sp, n]],  A^T g = (Spg, Sg);  det(A^T A) = n Cpp, without the cancellation of Spp n - Sp^2
    const double n = v.n, sp = n * v.mp, spp = v.cpp + sp * v.mp, sg = n * v.mg, spg = v.cpg + sp * v.mg;
    const double a = spp, b = sp, d = n, tr = a + d, det = n * v.cpp;
    const double disc = tr * tr / 4.0 - det;
    const double lmax = tr / 2.0 + sqrt(disc > 0.0 ? disc : 0.0);
    const double rc = 2.220446049250313e-16 * (n > 2.0 ? n : 2.0);        // np.linalg.lstsq(rcond=None): eps * max(M, N)
    double s = 0.0, t = 0.0;
    if (det > rc * rc * lmax * lmax) {                                     // sigma_min > rcond * sigma_max
        s = v.cpg / v.cpp;
        t = v.mg - s * v.mp;
    } else if (lmax > 0.0) {                                               // rank 1: the minimum-norm solution v (v . A^T g) / lambda_max
        double v0 = b, v1 = lmax - a;
        const double u0 = lmax - d, u1 = b;
        if (u0 * u0 + u1 * u1 > v0 * v0 + v1 * v1) { v0 = u0; v1 = u1; }
        const double nv = sqrt(v0 * v0 + v1 * v1);
        if (nv > 0.0) {
            v0 /= nv; v1 /= nv;
        } else {                                                           // b == 0 and a == d: any unit vector
            v0 = 1.0; v1 = 0.0;
        }
        const double c = (v0 * spg + v1 * sg) / lmax;
        s = v0 * c;
        t = v1 * c;
    }
    State *st = state(ws);
    st->scale = s;
    st->shift = t;
}

template <bool VEC>
__global__ __launch_bounds__(kSumThreads) void k_de_metrics(const float *gt, const float *pred, const uint8_t *mask, int64_t n, float dmin,
                                                            float dmax, int scaling, unsigned char *ws) {
#pragma clang fp contract(off)
    __shared__ double red[16];
    const State *st = state(ws);
    const double sc = st->scale, sh = st->shift, lo = dmin, hi = dmax;
    double s[kParts] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for_elems<VEC>(gt, pred, mask, n, [&](float gf, float pf, bool m) {
        if (!(m && gf > dmin && gf < dmax)) return;
        const double g = gf;
        double p = pf;
        if (scaling == BT_DEPTH_SCALE_MEDIAN) p = p * sc;
        else if (scaling == BT_DEPTH_SCALE_LSTSQ) p = sc * p + sh;
        if (p < lo) p = lo;                                               // (a NaN stays NaN, as numpy's masked assignment leaves it)
        if (p > hi) p = hi;
        const double r1 = g / p, r2 = p / g, th = r1 > r2 ? r1 : r2;     // np.maximum(gt / pred, pred / gt), exactly
        // log(g) - log(p) as log(g / p) and log10 as log / ln 10: one float64 log per element instead of four (the metric pass is
        // bound by the float64 pipe); within a few ulp of numpy's per element, far inside the 1e-9 the sums are held to
        const double e = g - p, q = e / g, l = log(r1);
        s[0] += fabs(q);
        s[1] += e * q;
        s[2] += fabs(l) * 0.43429448190325176;                           // 1 / ln 10
        s[3] += e * e;
        s[4] += l * l;
        s[5] += th < 1.25 ? 1.0 : 0.0;
        s[6] += th < 1.5625 ? 1.0 : 0.0;                                  // 1.25 ** 2
        s[7] += th < 1.953125 ? 1.0 : 0.0;                                // 1.25 ** 3
        s[8] += 1.0;
    });
    double *out = partials(ws) + (size_t)blockIdx.x * kParts;
    for (int q = 0; q < kParts; ++q) {
        const double t = block_sum_d(s[q], red);
        if (threadIdx.x == 0) out[q] = t;
    }
}

__global__ __launch_bounds__(256) void k_de_final(unsigned char *ws, int nb, double *out) {
    __shared__ double red[16];
    __shared__ double tot[kParts];
    const double *part = partials(ws);
    for (int q = 0; q < kParts; ++q) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nb; b += blockDim.x) v += part[(size_t)b * kParts + q];
        v = block_sum_d(v, red);
        if (threadIdx.x == 0) tot[q] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double c = tot[8];
    out[0] = tot[0] / c;
    out[1] = tot[1] / c;
    out[2] = tot[2] / c;
    out[3] = sqrt(tot[3] / c);
    out[4] = sqrt(tot[4] / c);
    out[5] = tot[5] / c;
    out[6] = tot[6] / c;
    out[7] = tot[7] / c;
    out[8] = c;
    const State *st = state(ws);
    out[9] = st->scale;
    out[10] = st->shift;
}

__global__ __launch_bounds__(256) void k_de_init(unsigned char *ws) {
    uint32_t *h = reinterpret_cast<uint32_t *>(ws);
    for (int i = threadIdx.x; i < kPasses * kSel * kBins; i += blockDim.x) h[i] = 0u;
    if (threadIdx.x == 0) {
        State *st = state(ws);
        for (int s = 0; s < kSel; ++s) { st->prefix[s] = 0u; st->rank[s] = 0u; }
        st->count = 0u;
        st->nan_pred = 0u;
        st->scale = 1.0;
        st->shift = 0.0;
    }
}

template <bool VEC>
void launch(const float *gt, const float *pred, const uint8_t *mask, int64_t n, float dmin, float dmax, int scaling, unsigned char *ws,
            double *out, hipStream_t st) {
    const int nbh = (int)(n / (4 * kHistThreads) + 1 < kHistBlocks ? n / (4 * kHistThreads) + 1 : kHistBlocks);
    const int nbs = (int)(n / (4 * kSumThreads) + 1 < kSumBlocks ? n / (4 * kSumThreads) + 1 : kSumBlocks);
    hipLaunchKernelGGL(k_de_init, dim3(1), dim3(256), 0, st, ws);
    if (scaling == BT_DEPTH_SCALE_MEDIAN) {
        for (int pass = 0; pass < kPasses; ++pass) {
            hipLaunchKernelGGL(k_de_hist<VEC>, dim3(nbh), dim3(kHistThreads), 0, st, gt, pred, mask, n, dmin, dmax, ws, pass);
            hipLaunchKernelGGL(k_de_pick, dim3(1), dim3(256), 0, st, ws, pass);
        }
    } else if (scaling == BT_DEPTH_SCALE_LSTSQ) {
        hipLaunchKernelGGL(k_de_sums<VEC>, dim3(nbs), dim3(kSumThreads), 0, st, gt, pred, mask, n, dmin, dmax, ws);
        hipLaunchKernelGGL(k_de_solve, dim3(1), dim3(256), 0, st, ws, nbs);
    }
    hipLaunchKernelGGL(k_de_metrics<VEC>, dim3(nbs), dim3(kSumThreads), 0, st, gt, pred, mask, n, dmin, dmax, scaling, ws);
    hipLaunchKernelGGL(k_de_final, dim3(1), dim3(256), 0, st, ws, nbs, out);
}

}  // namespace de
}  // namespace bt

extern "C" int64_t bt_depth_metrics_workspace_bytes(int64_t n) {
    if (n < 0) return BT_EINVAL;
    if (n > 0x7fffffffll) return BT_EUNSUPPORTED;
    return (int64_t)bt::de::kWsBytes;
}

extern "C" int bt_depth_metrics(const float *gt, const float *pred, const uint8_t *mask, int64_t n, float depth_min, float depth_max,
                                int32_t scaling, void *workspace, double *out, void *stream) {
    if (n < 0 || !gt || !pred || !workspace || !out) return BT_EINVAL;
    if (scaling != BT_DEPTH_SCALE_NONE && scaling != BT_DEPTH_SCALE_MEDIAN && scaling != BT_DEPTH_SCALE_LSTSQ) return BT_EINVAL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(out) & 7)) return BT_EINVAL;
    if (n > 0x7fffffffll) return BT_EUNSUPPORTED;
    const bool vec = (reinterpret_cast<uintptr_t>(gt) & 15) == 0 && (reinterpret_cast<uintptr_t>(pred) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec)
        bt::de::launch<true>(gt, pred, mask, n, depth_min, depth_max, scaling, ws, out, st);
    else
        bt::de::launch<false>(gt, pred, mask, n, depth_min, depth_max, scaling, ws, out, st);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
