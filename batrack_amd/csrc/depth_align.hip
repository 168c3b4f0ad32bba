// depth_align.hip — the reference's align_depth_maps (main/global_refine/model/utils.py:268-312) on gfx950
// (include/batrack_depth.h).  Frame i (i >= 1) is scaled by s = med_prev / med_cur, numpy's medians of
//   cur  = D[i][m],                                    m = (A[i-1] > 0) & (D[i] > 0),  c = |m|
//   prev = A[0][m] (i == 1)  or  A[i-2][(A[i-2] > 0) & (A[i-1] > 0)] ⊎ A[i-1][m]  (i >= 2)
// unless c < 100 (A[i] = D[i]).  Per frame, one fixed sequence of launches on the caller's stream, no host round trip:
//   k_ad_hist   one histogram pass of the radix select of radix_select.hpp (4 passes for float32, 8 for float64) over the
//               raw bits of the selected values (all > 0, so the bits order them), for four selections at once: the lower
//               and upper middle element of cur and of prev.
//   k_ad_pick   its pick, one workgroup, one wave per selection; clears the histogram for the next pass.
//               Pass 0 records c and the union count and decides the c < 100 branch; later passes of a skipped frame do
//               nothing.  The last pass forms the medians and s in the input's dtype and hands (s, skip) to the write pass.
//   k_ad_write  A[i] = s * D[i] (or D[i] for a skipped frame, or frame 0), 16-byte loads and stores, one multiply per pixel.
// Integer atomics only: a call repeats bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_depth.h"
#include "radix_select.hpp"

namespace bt {
namespace ad {

constexpr int kSel = 4;                          // cur lower, cur upper, prev lower, prev upper middle element
constexpr int kBins = rs::kBins;
constexpr int kHistThreads = 512, kHistBlocks = 256;
constexpr int kWriteThreads = 256, kWriteBlocks = 1024;
constexpr uint32_t kMinOverlap = 100;            // min_overlap_threshold, utils.py:273

struct State {
    uint64_t prefix[kSel];                       // key bits fixed so far (this frame)
    uint32_t rank[kSel];                         // rank still to find among the keys that carry the prefix
    uint32_t count[2];                           // c = |cur|, |prev|
    uint32_t skip;                               // this frame: c < 100
    uint32_t out_skip;                           // the last finished frame's branch and scale, read by its write pass
    double scale;
};

// workspace: histograms [kSel][kBins] uint32 (cleared by every pick) | State (256 B)
constexpr size_t kHistBytes = (size_t)kSel * kBins * sizeof(uint32_t);
constexpr size_t kStateOff = kHistBytes;
constexpr size_t kWsBytes = kStateOff + 256;
static_assert(sizeof(State) <= 256, "State");

using rs::mean2;

__device__ __forceinline__ State *state(unsigned char *ws) { return reinterpret_cast<State *>(ws + kStateOff); }
__device__ __forceinline__ const State *state(const unsigned char *ws) { return reinterpret_cast<const State *>(ws + kStateOff); }

__device__ __forceinline__ uint64_t key(float f) { return __float_as_uint(f); }          // f > 0: the raw bits order it
__device__ __forceinline__ uint64_t key(double f) { return (uint64_t)__double_as_longlong(f); }
template <class T> __device__ __forceinline__ T decode(uint64_t k);
template <> __device__ __forceinline__ float decode<float>(uint64_t k) { return __uint_as_float((uint32_t)k); }
template <> __device__ __forceinline__ double decode<double>(uint64_t k) { return __longlong_as_double((long long)k); }

// med_prev / med_cur in the dtype, correctly rounded: a float64 quotient of float32 operands rounds to float32 innocuously
// (53 >= 2 * 24 + 2), whatever the compiler's float32 division does
__device__ __forceinline__ float ratio(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ double ratio(double a, double b) { return a / b; }

template <class T> struct alignas(16) Vec { T v[16 / sizeof(T)]; };

// f(d, a1, a2) for every pixel of this thread's grid-stride share (D[i], A[i-1], A[i-2]; a2 = 0 without a past frame);
// 16-byte loads when VEC
template <class T, bool VEC, class F>
__device__ __forceinline__ void for_pixels(const T *cur, const T *prev, const T *past, int64_t n, F &&f) {
    const int64_t nth = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t start = 0;
    if (VEC) {
        constexpr int W = 16 / sizeof(T);
        const int64_t nv = n / W;
        for (int64_t i = tid; i < nv; i += nth) {
            const Vec<T> d = reinterpret_cast<const Vec<T> *>(cur)[i], a = reinterpret_cast<const Vec<T> *>(prev)[i];
            Vec<T> b{};
            if (past) b = reinterpret_cast<const Vec<T> *>(past)[i];
#pragma unroll
            for (int j = 0; j < W; ++j) f(d.v[j], a.v[j], b.v[j]);
        }
        start = W * nv;
    }
    for (int64_t i = start + tid; i < n; i += nth) f(cur[i], prev[i], past ? past[i] : T(0));
}

template <class T, bool VEC>
__global__ __launch_bounds__(kHistThreads) void k_ad_hist(const T *cur, const T *prev, const T *past, int64_t n, unsigned char *ws,
                                                          int pass) {
    const State *st = state(ws);
    if (pass > 0 && st->skip) return;                                     // c < 100: nothing to select
    __shared__ uint32_t h[kSel * kBins];
    rs::hist_clear(h, kSel * kBins);
    __syncthreads();
    constexpr int kBits = 8 * sizeof(T);
    const int shift = kBits - 8 - 8 * pass;
    const uint64_t hi = rs::fixed_mask<uint64_t>(pass, shift);
    const uint64_t p0 = st->prefix[0], p1 = st->prefix[1], p2 = st->prefix[2], p3 = st->prefix[3];
    for_pixels<T, VEC>(cur, prev, past, n, [&](T d, T a1, T a2) {
        const bool m = a1 > T(0) && d > T(0);                             // (NaN fails both tests)
        const bool mp = past != nullptr && a2 > T(0) && a1 > T(0);
        rs::add_pair(h, key(d), shift, hi, p0, p1, m);
        rs::add_pair(h + 2 * kBins, key(a1), shift, hi, p2, p3, m);
        rs::add_pair(h + 2 * kBins, key(a2), shift, hi, p2, p3, mp);
    });
    __syncthreads();
    rs::hist_flush(h, reinterpret_cast<uint32_t *>(ws), kSel * kBins);
}

template <class T>
__global__ __launch_bounds__(256) void k_ad_pick(unsigned char *ws, int pass, int64_t frame, double *scales, int64_t *overlap) {
    __shared__ uint64_t old[kSel], sel[kSel];
    __shared__ uint32_t tot[kSel];
    __shared__ uint32_t s_skip;
    constexpr int kPasses = sizeof(T);
    State *st = state(ws);
    uint32_t *gh = reinterpret_cast<uint32_t *>(ws);
    const int w = threadIdx.x >> 6;
    if (threadIdx.x < kSel) old[threadIdx.x] = sel[threadIdx.x] = st->prefix[threadIdx.x];   // old: as the histogram pass saw them
    if (threadIdx.x == 0) s_skip = pass == 0 ? 0u : st->skip;
    __syncthreads();
    if (!s_skip) {
        // pass 0: every element of a set is counted in its selections' histogram; the middle ranks of the set's size
        const uint32_t total = rs::narrow(gh + rs::shared_source(w, old) * kBins,
                                          [&](uint32_t t) { return pass == 0 ? rs::middle_rank(t, w & 1) : st->rank[w]; },
                                          8 * (kPasses - 1 - pass), sel[w], st->rank[w]);
        if ((threadIdx.x & 63) == 0) tot[w] = total;
    }
    __syncthreads();
    rs::hist_clear(gh, kSel * kBins);                                     // for the next pass (read above by this block only)
    if (threadIdx.x != 0) return;
    for (int q = 0; q < kSel; ++q) st->prefix[q] = sel[q];               // (the picks narrowed the copies in LDS)
    if (pass == 0) {
        st->count[0] = tot[0];
        st->count[1] = tot[2];
        st->skip = tot[0] < kMinOverlap ? 1u : 0u;
        if (kPasses > 1) return;
    }
    if (pass != kPasses - 1) return;
    const uint32_t c = st->count[0], np_ = st->count[1], skip = st->skip;
    double s = __builtin_nan("");
    if (!skip) {                                                           // c >= 100, so both sets hold an element
        const T cl = decode<T>(sel[0]), cu = decode<T>(sel[1]), pl = decode<T>(sel[2]), pu = decode<T>(sel[3]);
        const T med_cur = (c & 1u) ? cl : mean2(cl, cu);
        const T med_prev = (np_ & 1u) ? pl : mean2(pl, pu);
        s = (double)ratio(med_prev, med_cur);
    }
    st->scale = s;
    st->out_skip = skip;
    if (scales) scales[frame] = s;
    if (overlap) overlap[frame] = (int64_t)c;
    for (int q = 0; q < kSel; ++q) { st->prefix[q] = 0ull; st->rank[q] = 0u; }  // the next frame starts from here
    st->count[0] = st->count[1] = 0u;
    st->skip = 0u;
}

template <class T, bool VEC>
__global__ __launch_bounds__(kWriteThreads) void k_ad_write(const T *src, T *dst, int64_t n, const unsigned char *ws, int copy) {
#pragma clang fp contract(off)
    const State *st = state(ws);
    const bool cp = copy || st->out_skip;
    const T s = (T)st->scale;                                              // (exact: s was a T)
    const int64_t nth = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t start = 0;
    if (VEC) {
        constexpr int W = 16 / sizeof(T);
        const int64_t nv = n / W;
        for (int64_t i = tid; i < nv; i += nth) {
            Vec<T> d = reinterpret_cast<const Vec<T> *>(src)[i];
            if (!cp) {
#pragma unroll
                for (int j = 0; j < W; ++j) d.v[j] = s * d.v[j];
            }
            reinterpret_cast<Vec<T> *>(dst)[i] = d;
        }
        start = W * nv;
    }
    for (int64_t i = start + tid; i < n; i += nth) dst[i] = cp ? src[i] : s * src[i];
}

__global__ __launch_bounds__(256) void k_ad_init(unsigned char *ws, double *scales, int64_t *overlap) {
    uint32_t *h = reinterpret_cast<uint32_t *>(ws);
    for (int i = threadIdx.x; i < kSel * kBins; i += blockDim.x) h[i] = 0u;
    if (threadIdx.x == 0) {
        State *st = state(ws);
        for (int q = 0; q < kSel; ++q) { st->prefix[q] = 0ull; st->rank[q] = 0u; }
        st->count[0] = st->count[1] = 0u;
        st->skip = st->out_skip = 0u;
        st->scale = __builtin_nan("");
        if (scales) scales[0] = __builtin_nan("");
        if (overlap) overlap[0] = 0;
    }
}

template <class T, bool VEC>
void launch(const T *maps, T *aligned, int64_t nt, int64_t hw, double *scales, int64_t *overlap, unsigned char *ws, hipStream_t st) {
    const int64_t nv = VEC ? hw / (int64_t)(16 / sizeof(T)) : hw;
    const int nbh = (int)((nv + kHistThreads - 1) / kHistThreads < kHistBlocks ? (nv + kHistThreads - 1) / kHistThreads : kHistBlocks);
    const int nbw = (int)((nv + kWriteThreads - 1) / kWriteThreads < kWriteBlocks ? (nv + kWriteThreads - 1) / kWriteThreads : kWriteBlocks);
    hipLaunchKernelGGL(k_ad_init, dim3(1), dim3(256), 0, st, ws, scales, overlap);
    if (aligned != maps) hipLaunchKernelGGL((k_ad_write<T, VEC>), dim3(nbw), dim3(kWriteThreads), 0, st, maps, aligned, hw, ws, 1);
    for (int64_t i = 1; i < nt; ++i) {
        const T *cur = maps + i * hw, *prev = aligned + (i - 1) * hw, *past = i >= 2 ? aligned + (i - 2) * hw : nullptr;
        for (int pass = 0; pass < (int)sizeof(T); ++pass) {
            hipLaunchKernelGGL((k_ad_hist<T, VEC>), dim3(nbh), dim3(kHistThreads), 0, st, cur, prev, past, hw, ws, pass);
            hipLaunchKernelGGL(k_ad_pick<T>, dim3(1), dim3(256), 0, st, ws, pass, i, scales, overlap);
        }
        hipLaunchKernelGGL((k_ad_write<T, VEC>), dim3(nbw), dim3(kWriteThreads), 0, st, cur, aligned + i * hw, hw, ws, 0);
    }
}

template <class T>
void run(const void *maps, void *aligned, int64_t nt, int64_t hw, double *scales, int64_t *overlap, unsigned char *ws, hipStream_t st) {
    const bool vec = (reinterpret_cast<uintptr_t>(maps) & 15) == 0 && (reinterpret_cast<uintptr_t>(aligned) & 15) == 0 &&
                     (hw * (int64_t)sizeof(T)) % 16 == 0;                  // every frame's base 16-byte aligned
    const T *m = static_cast<const T *>(maps);
    T *a = static_cast<T *>(aligned);
    if (vec)
        launch<T, true>(m, a, nt, hw, scales, overlap, ws, st);
    else
        launch<T, false>(m, a, nt, hw, scales, overlap, ws, st);
}

}  // namespace ad
}  // namespace bt

extern "C" int64_t bt_align_depth_maps_workspace_bytes(int64_t hw, int32_t dtype) {
    if (hw < 1 || (dtype != BT_DEPTH_F32 && dtype != BT_DEPTH_F64)) return BT_EINVAL;
    if (hw >= (1ll << 30)) return BT_EUNSUPPORTED;
    return (int64_t)bt::ad::kWsBytes;
}

extern "C" int bt_align_depth_maps(const void *maps, void *aligned, int64_t T, int64_t hw, int32_t dtype, double *scales, int64_t *overlap,
                                   void *workspace, void *stream) {
    if (T < 1 || hw < 1 || (dtype != BT_DEPTH_F32 && dtype != BT_DEPTH_F64) || !maps || !aligned || !workspace) return BT_EINVAL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(scales) & 7) ||
        (reinterpret_cast<uintptr_t>(overlap) & 7))
        return BT_EINVAL;
    if (hw >= (1ll << 30)) return BT_EUNSUPPORTED;
    const int64_t es = dtype == BT_DEPTH_F64 ? 8 : 4;
    if (T > INT64_MAX / (hw * es)) return BT_EUNSUPPORTED;
    const uintptr_t m0 = reinterpret_cast<uintptr_t>(maps), a0 = reinterpret_cast<uintptr_t>(aligned), nb = (uintptr_t)(T * hw * es);
    const size_t esz = (size_t)es;
    if (m0 != a0 && m0 < a0 + nb && a0 < m0 + nb) return BT_EINVAL;       // in place, or apart
    if ((m0 | a0) % esz) return BT_EINVAL;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == BT_DEPTH_F64)
        bt::ad::run<double>(maps, aligned, T, hw, scales, overlap, ws, st);
    else
        bt::ad::run<float>(maps, aligned, T, hw, scales, overlap, ws, st);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
