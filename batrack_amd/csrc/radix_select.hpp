// radix_select.hpp — exact selection (order statistics) by an 8-bit radix select, most significant digit first; every piece of
// the step exists here once.  A pass histograms the digit at `shift` of the keys that carry the prefix fixed so far, then one
// wave per selection scans the 256 bins and narrows (prefix, rank).  Holds: order-preserving keys of float32 / float64 values
// (fkey, fdecode); the fixed-bits test (fixed_mask, carries); the wave-aggregated LDS histogram increment (hist_add), the pair
// of increments of a lower / upper middle selection (add_pair) next to its mirror on the pick side (shared_source); the LDS
// histogram's clear and flush (hist_clear, hist_flush); the pick (middle_rank, wave_scan, find_digit, narrow); numpy's mean of
// the two middle elements (mean2).  Used by depth_eval.hip (k_de_hist, k_de_pick), depth_align.hip (k_ad_hist, k_ad_pick),
// mono_align.hip (k_ma_hist, k_ma_pick, k_ma_scene) and observe.hip (k_observe_threshold).
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

// the key bits that the passes before `pass` have fixed (the digit of this pass sits at `shift`), and whether a key carries them
template <class K>
__device__ __forceinline__ K fixed_mask(int pass, int shift) {
    return pass == 0 ? K(0) : (K)(~K(0) << (shift + 8));
}
template <class K>
__device__ __forceinline__ bool carries(K key, K prefix, K mask) {
    return ((key ^ prefix) & mask) == K(0);
}

constexpr int kBins = 256;                       // of one selection's histogram

// Selections come in pairs, the lower (even w) and the upper (odd w) middle element of one set.  While the pair's prefixes agree
// (always on pass 0) their histograms would be equal, so only the lower one's is built (add_pair) and the upper selection reads
// that one (shared_source).  The two sides of one rule: both look at the prefixes as they were before the pass's pick.
template <class K>
__device__ __forceinline__ int shared_source(int w, const K *prefixes) {
    return ((w & 1) && prefixes[w] == prefixes[w - 1]) ? w - 1 : w;
}
// h: the pair's two histograms, [2][kBins]
template <class K>
__device__ __forceinline__ void add_pair(uint32_t *h, K key, int shift, K mask, K p_lo, K p_hi, bool act) {
    hist_add(h, key, shift, act && carries(key, p_lo, mask));
    if (!(p_lo == p_hi)) hist_add(h + kBins, key, shift, act && carries(key, p_hi, mask));
}

// a workgroup's histograms of n bins in all: the clear (the caller synchronises), and the flush of the non-zero bins to global memory
__device__ __forceinline__ void hist_clear(uint32_t *h, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) h[i] = 0u;
}
__device__ __forceinline__ void hist_flush(const uint32_t *h, uint32_t *gh, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&gh[i], c);
    }
}

// pass 0: the rank of the lower or the upper middle element of `total` elements
__device__ __forceinline__ uint32_t middle_rank(uint32_t total, bool upper) {
    return upper ? total / 2 : (total ? (total - 1) / 2 : 0u);
}

// one wave, 4 bins a lane: the inclusive / exclusive prefix of this lane's four bins and the histogram's total
__device__ __forceinline__ void wave_scan(const uint32_t *hh, uint32_t c[4], uint32_t &excl, uint32_t &inc, uint32_t &total) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = hh[4 * lane + j];
    const uint32_t loc = c[0] + c[1] + c[2] + c[3];
    inc = loc;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    excl = inc - loc;
    total = __shfl(inc, 63);
}

// in the lane whose bins hold rank k (excl <= k < inc): the digit, the rank left among the keys of that digit, and their count
__device__ __forceinline__ int find_digit(const uint32_t c[4], uint32_t excl, uint32_t k, uint32_t &rem, uint32_t &cnt) {
    const int lane = threadIdx.x & 63;
    uint32_t cum = excl;
    int d = 4 * lane + 3;
    cnt = c[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (k < cum + c[j]) { d = 4 * lane + j; cnt = c[j]; break; }
        cum += c[j];
    }
    rem = k - cum;
    return d;
}
__device__ __forceinline__ int find_digit(const uint32_t c[4], uint32_t excl, uint32_t k, uint32_t &rem) {
    uint32_t cnt;
    return find_digit(c, excl, k, rem, cnt);
}

// One wave's pick of a pass: scans the histogram hh, takes the rank to find from rank_of(total) (pass 0 knows its rank only from
// the total), and in the lane that holds it narrows (prefix, rank) to the digit's bin.  Every lane gets the total.
template <class K, class F>
__device__ __forceinline__ uint32_t narrow(const uint32_t *hh, F &&rank_of, int shift, K &prefix, uint32_t &rank) {
    uint32_t c[4], excl, inc, total;
    wave_scan(hh, c, excl, inc, total);
    const uint32_t k = rank_of(total);
    if (total > 0 && excl <= k && k < inc) {
        uint32_t rem;
        const int d = find_digit(c, excl, k, rem);
        prefix = prefix | ((K)d << shift);
        rank = rem;
    }
    return total;
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
