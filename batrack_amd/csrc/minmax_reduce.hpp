// minmax_reduce.hpp — the one copy of the (min, max) reduction that k_depth_range, k_window_depth (window_fmaps.hip) and
// k_frame_prep (video_prep.hip) end in, with the depth rule they share.
//
// Each block reduces its own share and leaves the pair in the workspace; a ticket tells the last block to finish that it is
// the last, and it reduces the pairs and puts the ticket back to zero.  One launch, no atomics on the values, and min / max
// do not depend on the order.  A NaN among the values makes both results NaN, as torch's min() and max() do.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace bt {

constexpr int WD_THREADS = 256;                                  // the block size minmax_finish is written for

__device__ __forceinline__ float depth_process(float d, int use_log) {
    if (!use_log) return d;
    return logf(d < 1e-3f ? 1e-3f : d);                        // clamp(min=1e-3): a NaN stays NaN
}

// torch's min / max: a NaN on either side is the result
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || b != b) ? NAN : fminf(a, b); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }
__device__ __forceinline__ void nan_minmax(float v, float &mn, float &mx) { mn = nan_min(mn, v); mx = nan_max(mx, v); }

// the depth range's rule for one raw depth d: selected when use_log or d > 0.01 (never a NaN then), processed, folded in
__device__ __forceinline__ void depth_range_fold(float d, int use_log, float &mn, float &mx) {
    if (use_log || d > 0.01f) nan_minmax(depth_process(d, use_log), mn, mx);
}

// the block's (mn, mx) -> part[block]; the last of the `blocks` blocks to arrive reduces part[0 .. blocks) into out[0 .. 1].
// Every thread of the block calls it; it may be called again (another ticket, another part) once it has returned.
__device__ inline void minmax_finish(float mn, float mx, float *part, unsigned *ticket, float *out, unsigned block, unsigned blocks) {
    __shared__ float s_mn[WD_THREADS / 64], s_mx[WD_THREADS / 64];
    __shared__ unsigned s_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto block_reduce = [&](float &a, float &b) {
        for (int o = 32; o; o >>= 1) { a = nan_min(a, __shfl_xor(a, o)); b = nan_max(b, __shfl_xor(b, o)); }
        __syncthreads();
        if (lane == 0) { s_mn[wave] = a; s_mx[wave] = b; }
        __syncthreads();
        a = s_mn[0]; b = s_mx[0];
        for (int i = 1; i < WD_THREADS / 64; ++i) { a = nan_min(a, s_mn[i]); b = nan_max(b, s_mx[i]); }
    };
    block_reduce(mn, mx);
    if (threadIdx.x == 0) {
        __hip_atomic_store(part + 2 * block, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part + 2 * block + 1, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        s_last = atomicAdd(ticket, 1u) == blocks - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    mn = INFINITY; mx = -INFINITY;
    for (unsigned i = threadIdx.x; i < blocks; i += WD_THREADS) {
        mn = nan_min(mn, __hip_atomic_load(part + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        mx = nan_max(mx, __hip_atomic_load(part + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    block_reduce(mn, mx);
    if (threadIdx.x == 0) {
        out[0] = mn; out[1] = mx;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace bt
