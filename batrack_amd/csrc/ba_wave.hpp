// ba_wave.hpp — wave-level device helpers shared by ba_tile.hip, ba_solve.hip, ba_etile.hip and the two-edges-per-lane kernels
// (ba_edge2.hpp): sums over groups and residue classes of lanes by DPP and lane swaps (float and double), the wavefront fence,
// wave-uniform values into SGPRs, the factorisations' reciprocal square root, 6-element rows as three vector accesses.
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

// ------------------------------------------------------------------ cross-lane sums, float and double
// x of the lane the DPP control names (a double as its two halves); `old` where the control leaves a lane unwritten
template <int CTRL, int BANK = 0xf, bool BOUND = true>
__device__ __forceinline__ float lane_dpp(float old, float x) {
    return __uint_as_float((unsigned)__builtin_amdgcn_update_dpp((int)__float_as_uint(old), (int)__float_as_uint(x), CTRL, 0xf, BANK, BOUND));
}
template <int CTRL, int BANK = 0xf, bool BOUND = true>
__device__ __forceinline__ double lane_dpp(double old, double x) {
    const unsigned long long o = (unsigned long long)__double_as_longlong(old), v = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)o, (int)(unsigned)v, CTRL, 0xf, BANK, BOUND);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(o >> 32), (int)(unsigned)(v >> 32), CTRL, 0xf, BANK, BOUND);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// x + (x of lane ^ 16), x + (x of lane ^ 32): v_permlane16_swap / v_permlane32_swap
__device__ __forceinline__ float lane_swap16(float x) {
    const uint2_t r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
__device__ __forceinline__ float lane_swap32(float x) {
    const uint2_t r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
__device__ __forceinline__ double lane_mk(unsigned lo, unsigned hi) { return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)); }
__device__ __forceinline__ double lane_swap16(double x) {
    const unsigned long long v = (unsigned long long)__double_as_longlong(x);
    const uint2_t rl = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    const uint2_t rh = __builtin_amdgcn_permlane16_swap((unsigned)(v >> 32), (unsigned)(v >> 32), false, false);
    return lane_mk(rl.x, rh.x) + lane_mk(rl.y, rh.y);
}
__device__ __forceinline__ double lane_swap32(double x) {
    const unsigned long long v = (unsigned long long)__double_as_longlong(x);
    const uint2_t rl = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    const uint2_t rh = __builtin_amdgcn_permlane32_swap((unsigned)(v >> 32), (unsigned)(v >> 32), false, false);
    return lane_mk(rl.x, rh.x) + lane_mk(rl.y, rh.y);
}
// x + (x of lane ^ M)
template <int M, typename T>
__device__ __forceinline__ T xor_add(T x) {
    if (M == 1) return x + lane_dpp<0xb1>((T)0, x);
    if (M == 2) return x + lane_dpp<0x4e>((T)0, x);
    if (M == 4) {
        T t = lane_dpp<0x104, 0x5, false>((T)0, x);           // row_shl:4 on the banks with bit 2 clear
        t = lane_dpp<0x114, 0xa, false>(t, x);                 // row_shr:4 on the others
        return x + t;
    }
    if (M == 8) return x + lane_dpp<0x128>((T)0, x);
    if (M == 16) return lane_swap16(x);
    return lane_swap32(x);
}
// sum of x over the groups of 2^lg adjacent lanes (every lane of a group gets the total); lg is wave-uniform.  Inside a row
// the partners are quad_perm (lane ^ 1, lane ^ 2), row_half_mirror (7 - lane of the 8) and row_mirror (15 - lane of the 16)
template <int N, typename T>
__device__ __forceinline__ void group_sum(T (&x)[N], int lg) {
    if (lg > 0) { _Pragma("unroll") for (int i = 0; i < N; ++i) x[i] += lane_dpp<0xb1>((T)0, x[i]); }
    if (lg > 1) { _Pragma("unroll") for (int i = 0; i < N; ++i) x[i] += lane_dpp<0x4e>((T)0, x[i]); }
    if (lg > 2) { _Pragma("unroll") for (int i = 0; i < N; ++i) x[i] += lane_dpp<0x141>((T)0, x[i]); }
    if (lg > 3) { _Pragma("unroll") for (int i = 0; i < N; ++i) x[i] += lane_dpp<0x140>((T)0, x[i]); }
    if (lg > 4) { _Pragma("unroll") for (int i = 0; i < N; ++i) x[i] = lane_swap16(x[i]); }
    if (lg > 5) { _Pragma("unroll") for (int i = 0; i < N; ++i) x[i] = lane_swap32(x[i]); }
}
// sum of x over the lanes with the same (lane mod 2^lg) (lane < 2^lg then holds the total of its residue class)
template <int N, typename T>
__device__ __forceinline__ void stride_sum(T (&x)[N], int lg) {
    if (lg <= 5) { _Pragma("unroll") for (int i = 0; i < N; ++i) x[i] = xor_add<32>(x[i]); }
    if (lg <= 4) { _Pragma("unroll") for (int i = 0; i < N; ++i) x[i] = xor_add<16>(x[i]); }
    if (lg <= 3) { _Pragma("unroll") for (int i = 0; i < N; ++i) x[i] = xor_add<8>(x[i]); }
    if (lg <= 2) { _Pragma("unroll") for (int i = 0; i < N; ++i) x[i] = xor_add<4>(x[i]); }
    if (lg <= 1) { _Pragma("unroll") for (int i = 0; i < N; ++i) x[i] = xor_add<2>(x[i]); }
    if (lg <= 0) { _Pragma("unroll") for (int i = 0; i < N; ++i) x[i] = xor_add<1>(x[i]); }
}
template <typename T>
__device__ __forceinline__ T dpp_add8(T v) {            // sum over aligned groups of 8 lanes, all lanes get it
    T x[1] = {v};
    group_sum(x, 3);
    return x[0];
}

__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// wave-uniform metadata: LDS -> SGPRs
__device__ __forceinline__ int4 uniform4(const int4 v) {
    return make_int4(__builtin_amdgcn_readfirstlane(v.x), __builtin_amdgcn_readfirstlane(v.y),
                     __builtin_amdgcn_readfirstlane(v.z), __builtin_amdgcn_readfirstlane(v.w));
}

}  // namespace bt
