// radix_select.hpp — the pieces the exact-median kernels share (depth_eval.hip, depth_align.hip, mono_align.hip): order-preserving
// keys of float32 / float64 values, the wave-aggregated LDS histogram increment of an 8-bit radix pass, and numpy's mean of the
// two middle elements of an even count.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bt {
namespace rs {

// order-preserving keys; -0 and +0 are one key, as numpy compares them.  (NaN gets a key too: the callers leave NaN out.)
__device__ __forceinline__ uint32_t fkey(float f) {
    uint32_t u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t fkey(double f) {
    uint64_t u = (uint64_t)__double_as_longlong(f);
    if (u == 0x8000000000000000ull) u = 0ull;
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ float fdecode(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ double fdecode(uint64_t k) {
    return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k));
}

// h[bin of key] += 1 for the lanes with `act`: the lanes that share the first active lane's bin add once, together (a tied or
// constant input then costs one LDS atomic per wave), the others one each
template <class K>
__device__ __forceinline__ void hist_add(uint32_t *h, K key, int shift, bool act) {
    const uint64_t am = __ballot(act);
    if (am == 0) return;
    const int bin = (int)((key >> shift) & 0xffu);
    const int leader = __ffsll((unsigned long long)am) - 1;
    const int lb = __shfl(bin, leader);
    const uint64_t same = __ballot(act && bin == lb);
    if (act) {
        if (bin != lb) atomicAdd(&h[bin], 1u);
        else if ((int)__lane_id() == leader) atomicAdd(&h[lb], (uint32_t)__popcll(same));
    }
}

// numpy's median of the two middle elements, np.mean in the dtype: float32 sums in float32 and divides by the count in float64
// (float32 / intp), which is exact halving rounded once; float64 sums and divides in float64
__device__ __forceinline__ float mean2(float lo, float hi) {
    const float s = lo + hi;
    return (float)((double)s / 2.0);
}
__device__ __forceinline__ double mean2(double lo, double hi) { return (lo + hi) / 2.0; }

}  // namespace rs
}  // namespace bt
