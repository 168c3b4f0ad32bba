// ba_wave.hpp — wave-level device helpers shared by ba_tile.hip and ba_solve.hip: DPP sums over groups of 8 lanes, the wavefront
// fence, wave-uniform values into SGPRs, the factorisations' reciprocal square root, 6-element rows as three vector accesses.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_edge.hpp"

namespace bt {

template <typename T> __device__ __forceinline__ T rsqrt_t(T x);
template <> __device__ __forceinline__ float rsqrt_t<float>(float x) { return rsqrtf(x); }
template <> __device__ __forceinline__ double rsqrt_t<double>(double x) {
    // fp32 hardware seed (1 ulp) + one Newton step in double: relative error ~1e-14.
    // A non-positive or NaN pivot is caught by the caller's (s > 0) test.
    const double y = (double)__builtin_amdgcn_rsqf((float)x);
    return y * (1.5 - 0.5 * x * y * y);
}

template <typename T>
__device__ __forceinline__ void load_row6(const T *p, T (&v)[6]) {
    typedef typename Vec2<T>::type V;
    const V a = reinterpret_cast<const V *>(p)[0], b = reinterpret_cast<const V *>(p)[1], c = reinterpret_cast<const V *>(p)[2];
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y; v[4] = c.x; v[5] = c.y;
}
template <typename T>
__device__ __forceinline__ void store_row6(T *p, const T (&v)[6]) {
    typedef typename Vec2<T>::type V;
    V a, b, c;
    a.x = v[0]; a.y = v[1]; b.x = v[2]; b.y = v[3]; c.x = v[4]; c.y = v[5];
    reinterpret_cast<V *>(p)[0] = a; reinterpret_cast<V *>(p)[1] = b; reinterpret_cast<V *>(p)[2] = c;
}

__device__ __forceinline__ float dpp_add8(float v) {   // sum over aligned groups of 8 lanes, all lanes get it
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));   // quad xor 1
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));   // quad xor 2
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true));  // row_half_mirror
    return v;
}
__device__ __forceinline__ double dpp_perm(double v, int sel) {
    const long long b = __double_as_longlong(v);
    int lo = (int)(b & 0xffffffffll), hi = (int)(b >> 32);
    if (sel == 0) { lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, true); }
    else if (sel == 1) { lo = __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xF, 0xF, true); }
    else { lo = __builtin_amdgcn_update_dpp(0, lo, 0x141, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x141, 0xF, 0xF, true); }
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double dpp_add8(double v) {
    v += dpp_perm(v, 0); v += dpp_perm(v, 1); v += dpp_perm(v, 2);
    return v;
}

__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// wave-uniform metadata: LDS -> SGPRs
__device__ __forceinline__ int4 uniform4(const int4 v) {
    return make_int4(__builtin_amdgcn_readfirstlane(v.x), __builtin_amdgcn_readfirstlane(v.y),
                     __builtin_amdgcn_readfirstlane(v.z), __builtin_amdgcn_readfirstlane(v.w));
}

}  // namespace bt
