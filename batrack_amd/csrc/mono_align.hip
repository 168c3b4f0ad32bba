// mono_align.hip — the reference's align_depth (main/mono_depth/get_mono_depth.py:21-150) on gfx950 (include/batrack_depth.h):
// relative mono disparity d (float32) to metric depth, given the metric depth m of the same frames, in m's dtype D as numpy
// computes it.  Per frame t
//   g = 1 / (m + 1e-8),  g = 1e-2 where (m < 2) & (d < 0.02)
//   s_t = median((g - median(g) + 1e-8) / (d - median(d) + 1e-8)),   c_t = median(g - s_t d)
// and across the scene
//   p = s c,  k = argmin |p - median(p)|,  y = s_k d + c_k,  n = percentile(y, 98) / 2,
//   depth = clip(1 / ((1 / n) y), 1e-4, 1e4),  depth = 0 where depth < 1e-2.
// One fixed sequence of launches on the caller's stream, no host round trip, nothing allocated:
//   k_ma_init    clears the histograms and the selection state (the workspace's contents on entry are arbitrary).
//   k_ma_hist    one histogram pass of the radix select of radix_select.hpp (4 passes for float32, 8 for float64), SEGMENTED:
//                a workgroup takes a slice of one frame and adds to that frame's histograms.  NaN is left out, so a segment's
//                NaN count is its size minus its histogram total.  g, the ratio and g - s d are recomputed from m and d in
//                every pass: storing g would cost the same bytes as reading m.
//                  round A   the two middle elements of g and of d, for every frame at once
//                  round B   the two middle elements of the ratio            round C   of g - s_t d
//                  round P   two order statistics of y over all T*H*W elements (numpy's previous / next index of the 98th
//                            percentile), one segment
//   k_ma_pick    its pick, one wave per selection (a workgroup per frame); clears the histogram for the next pass; the last
//                pass forms the medians (NaN when the segment holds a NaN) or the percentile's interpolation.
//   k_ma_scene   one workgroup: median(p) by radix select in LDS, the argmin (first index on ties, the first NaN if any), the
//                aligns and numpy's percentile indices and gamma for T*H*W elements.
//   k_ma_write   depth from d, 16-byte loads and stores.
// Every operation of the formulas is rounded once in D (#pragma clang fp contract(off); float32 divisions correctly rounded).
// Integer atomics only: a call repeats bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_depth.h"
#include "radix_select.hpp"

namespace bt {
namespace ma {

using rs::fdecode;
using rs::fkey;
using rs::mean2;

enum Round { kA = 0, kB = 1, kC = 2, kP = 3 };
constexpr int kBins = rs::kBins;
constexpr int kMaxSel = 4;                        // round A: g lower, g upper, d lower, d upper middle element
constexpr int kHistThreads = 512;
constexpr int kHistTarget = 2048;                 // workgroups of a hist pass: about 8 per CU, the rest grid-strided
constexpr int kPickThreads = 256, kPickBlocks = 4096;
constexpr int kSceneThreads = 1024;
constexpr int kWriteThreads = 256, kWriteBlocks = 2048;

struct Seg {                                      // the selections of one segment (a frame; the scene in round P)
    uint64_t prefix[kMaxSel];                     // key bits fixed so far
    uint32_t rank[kMaxSel];                       // rank still to find among the keys that carry the prefix
    uint32_t count[2];                            // non-NaN elements of the set(s), from pass 0
    uint32_t pad[2];
    double v[4];                                  // a frame's median(g), median(d), s, c (each exact in double)
};

struct Scene {
    Seg sel;                                      // round P
    int64_t target[2];                            // the percentile's ranks (numpy's previous / next index; -1 is the last)
    double gamma, a_s, a_c, inv_n;
    int64_t k;
};

// workspace: histograms [T][kMaxSel][kBins] uint32 (cleared by every pick; round P uses frame 0's) | Scene (512 B) | Seg [T]
constexpr size_t kSegHist = (size_t)kMaxSel * kBins * sizeof(uint32_t);
constexpr size_t kSceneBytes = 512;
static_assert(sizeof(Scene) <= kSceneBytes, "Scene");
static_assert(sizeof(Seg) % 16 == 0, "Seg");

__host__ __device__ inline size_t scene_off(int64_t nt) { return (size_t)nt * kSegHist; }
__host__ __device__ inline size_t segs_off(int64_t nt) { return scene_off(nt) + kSceneBytes; }
inline size_t ws_bytes(int64_t nt) { return (segs_off(nt) + (size_t)nt * sizeof(Seg) + 255) & ~(size_t)255; }

__device__ __forceinline__ uint32_t *hist(unsigned char *ws, int64_t s) { return reinterpret_cast<uint32_t *>(ws + (size_t)s * kSegHist); }
__device__ __forceinline__ Scene *scene(unsigned char *ws, int64_t nt) { return reinterpret_cast<Scene *>(ws + scene_off(nt)); }
__device__ __forceinline__ Seg *segs(unsigned char *ws, int64_t nt) { return reinterpret_cast<Seg *>(ws + segs_off(nt)); }

// the reference's Python scalars as numpy rounds them into D (NEP 50: a Python float takes the array's dtype)
template <class T> struct K;
template <> struct K<float> {
    static constexpr float eps = 1e-8f, fill = 1e-2f, lo = 1e-4f, hi = 1e4f, zero_below = 1e-2f;
};
template <> struct K<double> {
    static constexpr double eps = 1e-8, fill = 1e-2, lo = 1e-4, hi = 1e4, zero_below = 1e-2;
};

// a / b in the dtype, correctly rounded: a float64 quotient of float32 operands rounds to float32 innocuously (53 >= 2 * 24 + 2)
__device__ __forceinline__ float div(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ double div(double a, double b) { return a / b; }

// the per-pixel values of the formulas; d is float32, D the metric's dtype (a float32 d widens exactly)
template <class T>
__device__ __forceinline__ T gdisp(T m, float d) {
#pragma clang fp contract(off)
    T g = div(T(1), m + K<T>::eps);
    if (m < T(2) && d < 0.02f) g = K<T>::fill;                          // d < float32(0.02): numpy compares in float32
    return g;
}
template <class T>
__device__ __forceinline__ T ratio(T g, float d, T mg, float md) {
#pragma clang fp contract(off)
    const T num = (g - mg) + K<T>::eps;
    const float den = (d - md) + 1e-8f;                                  // float32 throughout (d and its median are float32)
    return div(num, (T)den);
}
template <class T>
__device__ __forceinline__ T resid(T g, float d, T s) {
#pragma clang fp contract(off)
    const T sd = s * (T)d;
    return g - sd;
}
template <class T>
__device__ __forceinline__ T affine(float d, T a_s, T a_c) {
#pragma clang fp contract(off)
    const T sd = a_s * (T)d;
    return sd + a_c;
}

template <class T> using Key = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;

template <class T> __device__ __forceinline__ void load4(const T *p, int64_t i, T v[4]);
template <> __device__ __forceinline__ void load4<float>(const float *p, int64_t i, float v[4]) {
    const float4 a = reinterpret_cast<const float4 *>(p)[i];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
template <> __device__ __forceinline__ void load4<double>(const double *p, int64_t i, double v[4]) {
    const double2 a = reinterpret_cast<const double2 *>(p)[2 * i], b = reinterpret_cast<const double2 *>(p)[2 * i + 1];
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}
template <class T> __device__ __forceinline__ void store4(T *p, int64_t i, const T v[4]);
template <> __device__ __forceinline__ void store4<float>(float *p, int64_t i, const float v[4]) {
    reinterpret_cast<float4 *>(p)[i] = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void store4<double>(double *p, int64_t i, const double v[4]) {
    reinterpret_cast<double2 *>(p)[2 * i] = make_double2(v[0], v[1]);
    reinterpret_cast<double2 *>(p)[2 * i + 1] = make_double2(v[2], v[3]);
}

// f(d, m) for the elements [0, len) of one segment that fall to `part` of `parts` slices (thread-strided); 16-byte loads (four
// elements of d, and of m when it is read) when VEC.  m == nullptr: m reads as 0.
template <class T, bool VEC, class F>
__device__ __forceinline__ void for_segment(const float *d, const T *m, int64_t len, int part, int parts, F &&f) {
    const int64_t nth = (int64_t)parts * blockDim.x, tid = (int64_t)part * blockDim.x + threadIdx.x;
    int64_t start = 0;
    if (VEC) {
        const int64_t nv = len >> 2;
        for (int64_t i = tid; i < nv; i += nth) {
            float dv[4];
            T mv[4] = {T(0), T(0), T(0), T(0)};
            load4<float>(d, i, dv);
            if (m) load4<T>(m, i, mv);
#pragma unroll
            for (int j = 0; j < 4; ++j) f(dv[j], mv[j]);
        }
        start = 4 * nv;
    }
    for (int64_t i = start + tid; i < len; i += nth) f(d[i], m ? m[i] : T(0));
}

template <class T, int R, bool VEC>
__global__ __launch_bounds__(kHistThreads) void k_ma_hist(const float *mono, const T *metric, int64_t nt, int64_t nseg, int64_t len,
                                                          int parts, unsigned char *ws, int pass) {
#pragma clang fp contract(off)
    constexpr int kSel = R == kA ? 4 : 2;
    __shared__ uint32_t h[kSel * kBins];
    const int shift = 8 * (int)sizeof(T) - 8 - 8 * pass;
    const uint64_t hi = rs::fixed_mask<uint64_t>(pass, shift);
    Scene *sc = scene(ws, nt);
    const Seg *sg_all = segs(ws, nt);
    const int64_t units = nseg * parts;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t s = u / parts;
        const int part = (int)(u - s * parts);
        rs::hist_clear(h, kSel * kBins);
        __syncthreads();
        const Seg *sg = R == kP ? &sc->sel : &sg_all[s];
        const uint64_t p0 = sg->prefix[0], p1 = sg->prefix[1], p2 = sg->prefix[2], p3 = sg->prefix[3];
        const float *d = mono + s * len;
        const T *m = R == kP ? nullptr : metric + s * len;
        // (a NaN value fails x == x and is never added: the histogram total of a set is its non-NaN count)
        auto add2 = [&](uint32_t *hh, T x, uint64_t q0, uint64_t q1) { rs::add_pair(hh, (uint64_t)fkey(x), shift, hi, q0, q1, x == x); };
        if (R == kA) {
            for_segment<T, VEC>(d, m, len, part, parts, [&](float dv, T mv) {
                add2(h, gdisp<T>(mv, dv), p0, p1);
                add2(h + 2 * kBins, (T)dv, p2, p3);                      // d's keys in D's width: the same order
            });
        } else if (R == kB) {
            const T mg = (T)sg->v[0];
            const float md = (float)sg->v[1];
            for_segment<T, VEC>(d, m, len, part, parts, [&](float dv, T mv) { add2(h, ratio<T>(gdisp<T>(mv, dv), dv, mg, md), p0, p1); });
        } else if (R == kC) {
            const T st = (T)sg->v[2];
            for_segment<T, VEC>(d, m, len, part, parts, [&](float dv, T mv) { add2(h, resid<T>(gdisp<T>(mv, dv), dv, st), p0, p1); });
        } else {
            const T a_s = (T)sc->a_s, a_c = (T)sc->a_c;
            for_segment<T, VEC>(d, (const T *)nullptr, len, part, parts, [&](float dv, T) { add2(h, affine<T>(dv, a_s, a_c), p0, p1); });
        }
        __syncthreads();
        rs::hist_flush(h, hist(ws, s), kSel * kBins);
        __syncthreads();                                                  // h is cleared for the next unit
    }
}

// numpy's median from the two middle elements of a set of `len` elements of which `count` are not NaN
template <class T> __device__ __forceinline__ T median_of(T lo, T hi, uint32_t count, int64_t len) {
    if ((int64_t)count != len) return T(__builtin_nan(""));
    return (len & 1) ? lo : mean2(lo, hi);
}

// numpy's _lerp(a, b, t): a + (b - a) t, or b - (b - a)(1 - t) where t >= 0.5
template <class T> __device__ __forceinline__ T lerp(T a, T b, T t) {
#pragma clang fp contract(off)
    const T diff = b - a;
    if (t >= T(0.5)) {
        const T w = diff * (T(1) - t);
        return b - w;
    }
    const T w = diff * t;
    return a + w;
}

template <class T, int R>
__global__ __launch_bounds__(kPickThreads) void k_ma_pick(unsigned char *ws, int64_t nt, int64_t nseg, int64_t len, int pass, T *frame_scale,
                                                          T *frame_shift, T *aligns) {
#pragma clang fp contract(off)
    constexpr int kSel = R == kA ? 4 : 2;
    constexpr int kPasses = sizeof(T);
    __shared__ uint64_t old[kMaxSel], sel[kMaxSel];
    __shared__ uint32_t tot[kMaxSel];
    Scene *sc = scene(ws, nt);
    const int w = threadIdx.x >> 6;
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        Seg *sg = R == kP ? &sc->sel : &segs(ws, nt)[s];
        uint32_t *gh = hist(ws, s);
        if (threadIdx.x < kSel) old[threadIdx.x] = sel[threadIdx.x] = sg->prefix[threadIdx.x];   // old: as the hist pass saw them
        __syncthreads();
        if (w < kSel) {
            auto rank_of = [&](uint32_t total) -> uint32_t {
                if (pass > 0) return sg->rank[w];
                if (R == kP) return total ? (uint32_t)((uint64_t)sc->target[w] < total ? sc->target[w] : total - 1) : 0u;
                return rs::middle_rank(total, w & 1);                     // of the non-NaN count
            };
            const uint32_t total = rs::narrow(gh + rs::shared_source(w, old) * kBins, rank_of, 8 * (kPasses - 1 - pass), sel[w], sg->rank[w]);
            if ((threadIdx.x & 63) == 0) tot[w] = total;
        }
        __syncthreads();
        rs::hist_clear(gh, kSel * kBins);                                 // for the next pass (read above by this block only)
        if (threadIdx.x == 0) {
            for (int q = 0; q < kSel; ++q) sg->prefix[q] = sel[q];       // (the picks narrowed the copies in LDS)
            if (pass == 0) {
                sg->count[0] = tot[0];
                sg->count[1] = kSel == 4 ? tot[2] : 0u;
            }
            if (pass == kPasses - 1) {
                using KT = Key<T>;
                const T lo = fdecode((KT)sel[0]), hi = fdecode((KT)sel[1]);
                const uint32_t cnt = pass == 0 ? tot[0] : sg->count[0];
                if (R == kA) {
                    const uint32_t cd = pass == 0 ? tot[2] : sg->count[1];
                    sg->v[0] = (double)median_of<T>(lo, hi, cnt, len);
                    sg->v[1] = (double)median_of<float>((float)fdecode((KT)sel[2]), (float)fdecode((KT)sel[3]), cd, len);
                } else if (R == kB) {
                    const T st = median_of<T>(lo, hi, cnt, len);
                    sg->v[2] = (double)st;
                    if (frame_scale) frame_scale[s] = st;
                } else if (R == kC) {
                    const T ct = median_of<T>(lo, hi, cnt, len);
                    sg->v[3] = (double)ct;
                    if (frame_shift) frame_shift[s] = ct;
                } else {
                    T r = lerp<T>(lo, hi, (T)sc->gamma);
                    if ((int64_t)cnt != len) r = T(__builtin_nan(""));            // numpy returns the last (a NaN) element
                    const T n = r / T(2);
                    sc->inv_n = (double)div(T(1), n);
                    if (aligns) aligns[2] = n;
                }
                for (int q = 0; q < kMaxSel; ++q) { sg->prefix[q] = 0ull; sg->rank[q] = 0u; }   // the next round starts here
                sg->count[0] = sg->count[1] = 0u;
            }
        }
        __syncthreads();                                                  // old / sel / tot are reused by the next segment
    }
}

// numpy's percentile(., 98) indices for n elements (method 'linear', numpy 2.x): q = D(98) / D(100), v = (n - 1) q in D (n - 1
// rounds to D first), previous = floor(v), next = previous + 1 in D; v >= n - 1 takes the last element for both (-1), and
// gamma = v - previous (a float64 difference of D and an integer, back in D)
template <class T> __device__ __forceinline__ void percentile_index(int64_t n, int64_t &prev, int64_t &next, T &gamma) {
#pragma clang fp contract(off)
    const T q = div(T(98), T(100));
    const T n1 = (T)(double)(n - 1);                                    // (exact in double, then rounded once)
    const T v = n1 * q;
    const T pf = floor(v);
    const T nf = pf + T(1);
    prev = (int64_t)pf;
    next = (int64_t)nf;
    if (v >= n1) prev = next = -1;
    gamma = (T)((double)v - (double)prev);
}

template <class T>
__global__ __launch_bounds__(kSceneThreads) void k_ma_scene(unsigned char *ws, int64_t nt, int64_t n, T *aligns, int64_t *med_index) {
#pragma clang fp contract(off)
    using KT = Key<T>;
    constexpr int kPasses = sizeof(T);
    __shared__ uint32_t h[2 * kBins];
    __shared__ uint64_t prefix[2];
    __shared__ uint32_t rank[2], total;
    __shared__ T red_v[kSceneThreads / 64];
    __shared__ int64_t red_i[kSceneThreads / 64];
    const Seg *sg = segs(ws, nt);
    Scene *sc = scene(ws, nt);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    auto pval = [&](int64_t t) { return (T)sg[t].v[2] * (T)sg[t].v[3]; };           // p = s c in D
    if (threadIdx.x < 2) { prefix[threadIdx.x] = 0ull; rank[threadIdx.x] = 0u; }
    // median(p): the two middle elements by radix select over the T values, in LDS
    for (int pass = 0; pass < kPasses; ++pass) {
        const int shift = 8 * kPasses - 8 - 8 * pass;
        const uint64_t hi = rs::fixed_mask<uint64_t>(pass, shift);
        rs::hist_clear(h, 2 * kBins);
        __syncthreads();
        const uint64_t q[2] = {prefix[0], prefix[1]};                     // as this pass's histograms see them
        for (int64_t t0 = 0; t0 < nt; t0 += blockDim.x) {                 // (whole waves run every trip: hist_add is wave-wide)
            const int64_t t = t0 + threadIdx.x;
            const bool in = t < nt;
            const T x = in ? pval(t) : T(0);
            rs::add_pair(h, (uint64_t)fkey(x), shift, hi, q[0], q[1], in && x == x);
        }
        __syncthreads();
        if (w < 2) {
            const uint32_t tt = rs::narrow(h + rs::shared_source(w, q) * kBins,
                                           [&](uint32_t t) { return pass > 0 ? rank[w] : rs::middle_rank(t, w & 1); }, shift, prefix[w], rank[w]);
            if (pass == 0 && threadIdx.x == 0) total = tt;
        }
        __syncthreads();
    }
    const T med = median_of<T>(fdecode((KT)prefix[0]), fdecode((KT)prefix[1]), total, nt);
    // argmin |p - median(p)|: numpy's first NaN if there is one, else the first minimum
    T bv = T(0);
    int64_t bi = -1;
    auto better = [](T v, int64_t i, T bv, int64_t bi) {               // (v, i) before (bv, bi) in numpy's argmin order
        if (bi < 0) return i >= 0;
        if (i < 0) return false;
        const bool vn = v != v, bn = bv != bv;
        if (vn != bn) return vn;
        if (vn) return i < bi;
        return v < bv || (v == bv && i < bi);
    };
    for (int64_t t = threadIdx.x; t < nt; t += blockDim.x) {
        const T dist = fabs(pval(t) - med);
        if (better(dist, t, bv, bi)) { bv = dist; bi = t; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const T ov = __shfl_xor(bv, o);
        const int64_t oi = __shfl_xor(bi, o);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { red_v[w] = bv; red_i[w] = bi; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int q = 1; q < (int)(blockDim.x / 64); ++q)
        if (better(red_v[q], red_i[q], bv, bi)) { bv = red_v[q]; bi = red_i[q]; }
    const int64_t k = bi < 0 ? 0 : bi;
    const T a_s = (T)sg[k].v[2], a_c = (T)sg[k].v[3];
    sc->k = k;
    sc->a_s = (double)a_s;
    sc->a_c = (double)a_c;
    int64_t prev, next;
    T gamma;
    percentile_index<T>(n, prev, next, gamma);
    sc->target[0] = prev < 0 ? n - 1 : prev;
    sc->target[1] = next < 0 ? n - 1 : (next > n - 1 ? n - 1 : next);
    sc->gamma = (double)gamma;
    if (aligns) { aligns[0] = a_s; aligns[1] = a_c; }
    if (med_index) *med_index = k;
}

template <class T, bool VEC>
__global__ __launch_bounds__(kWriteThreads) void k_ma_write(const float *mono, T *out, int64_t n, unsigned char *ws, int64_t nt) {
#pragma clang fp contract(off)
    const Scene *sc = scene(ws, nt);
    const T a_s = (T)sc->a_s, a_c = (T)sc->a_c, inv = (T)sc->inv_n;
    auto depth = [&](float d) {
        T x = div(T(1), inv * affine<T>(d, a_s, a_c));
        if (x == x) {                                                     // np.clip keeps a NaN
            if (x < K<T>::lo) x = K<T>::lo;
            if (x > K<T>::hi) x = K<T>::hi;
        }
        return x < K<T>::zero_below ? T(0) : x;
    };
    const int64_t nth = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t start = 0;
    if (VEC) {
        const int64_t nv = n >> 2;
        for (int64_t i = tid; i < nv; i += nth) {
            float dv[4];
            T o[4];
            load4<float>(mono, i, dv);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = depth(dv[j]);
            store4<T>(out, i, o);
        }
        start = 4 * nv;
    }
    for (int64_t i = start + tid; i < n; i += nth) out[i] = depth(mono[i]);
}

__global__ __launch_bounds__(256) void k_ma_init(unsigned char *ws, int64_t nt) {
    const int64_t nth = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t *h = reinterpret_cast<uint32_t *>(ws);
    const int64_t nh = nt * (int64_t)(kSegHist / sizeof(uint32_t));
    for (int64_t i = tid; i < nh; i += nth) h[i] = 0u;
    Seg *sg = segs(ws, nt);
    for (int64_t t = tid; t < nt; t += nth) {
        for (int q = 0; q < kMaxSel; ++q) { sg[t].prefix[q] = 0ull; sg[t].rank[q] = 0u; }
        sg[t].count[0] = sg[t].count[1] = 0u;
        for (int q = 0; q < 4; ++q) sg[t].v[q] = 0.0;
    }
    if (tid == 0) {
        Scene *sc = scene(ws, nt);
        for (int q = 0; q < kMaxSel; ++q) { sc->sel.prefix[q] = 0ull; sc->sel.rank[q] = 0u; }
        sc->sel.count[0] = sc->sel.count[1] = 0u;
        sc->target[0] = sc->target[1] = 0;
        sc->gamma = sc->a_s = sc->a_c = sc->inv_n = 0.0;
        sc->k = 0;
    }
}

inline int grid_for(int64_t units, int cap) { return (int)(units < cap ? units : cap); }

// workgroups per segment: enough for about kHistTarget in all, at least one, and no more than one per 4 * kHistThreads elements
inline int parts_for(int64_t nseg, int64_t len) {
    const int64_t want = (kHistTarget + nseg - 1) / nseg, most = (len + 4 * kHistThreads - 1) / (4 * kHistThreads);
    const int64_t p = want < most ? want : most;
    return (int)(p < 1 ? 1 : p);
}

template <class T, int R, bool VEC>
void round_passes(const float *mono, const T *metric, int64_t nt, int64_t nseg, int64_t len, unsigned char *ws, T *fs, T *fc, T *al,
                  hipStream_t st) {
    const int parts = parts_for(nseg, len);
    const int gh = grid_for(nseg * parts, 65536), gp = grid_for(nseg, kPickBlocks);
    for (int pass = 0; pass < (int)sizeof(T); ++pass) {
        hipLaunchKernelGGL((k_ma_hist<T, R, VEC>), dim3(gh), dim3(kHistThreads), 0, st, mono, metric, nt, nseg, len, parts, ws, pass);
        hipLaunchKernelGGL((k_ma_pick<T, R>), dim3(gp), dim3(kPickThreads), 0, st, ws, nt, nseg, len, pass, fs, fc, al);
    }
}

template <class T>
void run(const float *mono, const T *metric, int64_t nt, int64_t hw, T *out, T *fs, T *fc, T *al, int64_t *k, unsigned char *ws, hipStream_t st) {
    const int64_t n = nt * hw;
    const bool in16 = (reinterpret_cast<uintptr_t>(mono) & 15) == 0 && (reinterpret_cast<uintptr_t>(metric) & 15) == 0;
    const bool vf = in16 && (hw & 3) == 0;                               // every frame's base 16-byte aligned
    const bool vs = (reinterpret_cast<uintptr_t>(mono) & 15) == 0;
    const bool vw = vs && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    hipLaunchKernelGGL(k_ma_init, dim3(grid_for((nt * 1024 + 255) / 256, 1024)), dim3(256), 0, st, ws, nt);
    if (vf) {
        round_passes<T, kA, true>(mono, metric, nt, nt, hw, ws, fs, fc, al, st);
        round_passes<T, kB, true>(mono, metric, nt, nt, hw, ws, fs, fc, al, st);
        round_passes<T, kC, true>(mono, metric, nt, nt, hw, ws, fs, fc, al, st);
    } else {
        round_passes<T, kA, false>(mono, metric, nt, nt, hw, ws, fs, fc, al, st);
        round_passes<T, kB, false>(mono, metric, nt, nt, hw, ws, fs, fc, al, st);
        round_passes<T, kC, false>(mono, metric, nt, nt, hw, ws, fs, fc, al, st);
    }
    hipLaunchKernelGGL(k_ma_scene<T>, dim3(1), dim3(kSceneThreads), 0, st, ws, nt, n, al, k);
    if (vs)
        round_passes<T, kP, true>(mono, metric, nt, 1, n, ws, fs, fc, al, st);
    else
        round_passes<T, kP, false>(mono, metric, nt, 1, n, ws, fs, fc, al, st);
    const int gw = grid_for(((vw ? n / 4 : n) + kWriteThreads - 1) / kWriteThreads, kWriteBlocks);
    if (vw)
        hipLaunchKernelGGL((k_ma_write<T, true>), dim3(gw < 1 ? 1 : gw), dim3(kWriteThreads), 0, st, mono, out, n, ws, nt);
    else
        hipLaunchKernelGGL((k_ma_write<T, false>), dim3(gw < 1 ? 1 : gw), dim3(kWriteThreads), 0, st, mono, out, n, ws, nt);
}

inline bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

}  // namespace ma
}  // namespace bt

extern "C" int64_t bt_mono_align_workspace_bytes(int64_t T, int64_t hw, int32_t dtype) {
    if (T < 1 || hw < 1 || (dtype != BT_DEPTH_F32 && dtype != BT_DEPTH_F64)) return BT_EINVAL;
    if (T > 0x7fffffffll / hw) return BT_EUNSUPPORTED;
    return (int64_t)bt::ma::ws_bytes(T);
}

extern "C" int bt_mono_align(const float *mono, const void *metric, int64_t T, int64_t hw, int32_t dtype, void *depth_out, void *frame_scale,
                             void *frame_shift, void *aligns, int64_t *med_index, void *workspace, void *stream) {
    using bt::ma::overlap;
    if (T < 1 || hw < 1 || (dtype != BT_DEPTH_F32 && dtype != BT_DEPTH_F64) || !mono || !metric || !depth_out || !workspace) return BT_EINVAL;
    if (T > 0x7fffffffll / hw) return BT_EUNSUPPORTED;
    const size_t es = dtype == BT_DEPTH_F64 ? 8 : 4, n = (size_t)(T * hw);
    const uintptr_t mis = (reinterpret_cast<uintptr_t>(mono) & 3) | (reinterpret_cast<uintptr_t>(workspace) & 15) |
                          ((reinterpret_cast<uintptr_t>(metric) | reinterpret_cast<uintptr_t>(depth_out) | reinterpret_cast<uintptr_t>(frame_scale) |
                            reinterpret_cast<uintptr_t>(frame_shift) | reinterpret_cast<uintptr_t>(aligns)) % es) |
                          (reinterpret_cast<uintptr_t>(med_index) & 7);
    if (mis) return BT_EINVAL;
    const void *in[2] = {mono, metric};
    const size_t in_n[2] = {n * 4, n * es};
    const void *outs[6] = {depth_out, frame_scale, frame_shift, aligns, med_index, workspace};
    const size_t out_n[6] = {n * es, (size_t)T * es, (size_t)T * es, 3 * es, 8, bt::ma::ws_bytes(T)};
    for (int o = 0; o < 6; ++o)
        for (int i = 0; i < 2; ++i)
            if (overlap(outs[o], out_n[o], in[i], in_n[i])) return BT_EINVAL;
    for (int o = 0; o < 5; ++o)                                           // and nothing the call writes meets the workspace
        if (overlap(outs[o], out_n[o], workspace, out_n[5])) return BT_EINVAL;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == BT_DEPTH_F64)
        bt::ma::run<double>(mono, static_cast<const double *>(metric), T, hw, static_cast<double *>(depth_out), static_cast<double *>(frame_scale),
                            static_cast<double *>(frame_shift), static_cast<double *>(aligns), med_index, ws, st);
    else
        bt::ma::run<float>(mono, static_cast<const float *>(metric), T, hw, static_cast<float *>(depth_out), static_cast<float *>(frame_scale),
                           static_cast<float *>(frame_shift), static_cast<float *>(aligns), med_index, ws, st);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
