// sample_taps.hpp — the two pieces of sampling arithmetic that more than one kernel must reproduce bit for bit, one copy each:
//   blend4            the reference's patchify blend (backend/altcorr/correlation.py:55-66): the four weights from the
//                     fractional offsets, every product rounded, the sum left to right.       k_patchify<true>, k_patch_generate
//   bilinear_clamped  bilinear_sample2d (frontend/core/model_utils.py:75-158) of one map: floor, indices clamped to the
//                     map, weights from the unclamped corners, the sum left to right.        k_observe_query, k_patch_generate
//                     bilinear_taps + bilinear_blend are its two halves, for a point with many channels.        k_feat_sample
// Every operation is rounded (contraction off inside each function, whatever the including file sets); the division is the
// correctly rounded one: files that include this must not be built with a fast-math flag.
#pragma once
#include <hip/hip_runtime.h>

namespace bt {

// ((1-dy)(1-dx)) p00 + ((1-dy) dx) p01 + (dy (1-dx)) p10 + (dy dx) p11, same association as correlation.py:61-66
__device__ __forceinline__ float blend4(float dx, float dy, float p00, float p01, float p10, float p11) {
#pragma clang fp contract(off)
    const float w00 = (1.0f - dy) * (1.0f - dx), w01 = (1.0f - dy) * dx;
    const float w10 = dy * (1.0f - dx), w11 = dy * dx;
    const float t00 = w00 * p00, t01 = w01 * p01, t10 = w10 * p10, t11 = w11 * p11;     // products rounded, then summed
    return ((t00 + t01) + t10) + t11;
}

// torch's clamp(min=1e-2): a NaN stays NaN (fmaxf would return 1e-2)
__device__ __forceinline__ float clamp_min_1e2(float d) { return d < 1e-2f ? 1e-2f : d; }

// floor(x).int() with the out-of-range cases spelt out.  The reference converts on an x86 host, where every value that does
// not fit an int32 — beyond 2^31 on EITHER side, and NaN — becomes INT_MIN; so does this (a saturating conversion would put
// +3e9 at INT_MAX: other weights, another clamped index).  The largest float below 2^31 is 2^31 - 128: x0 + 1 never overflows.
__device__ __forceinline__ int floor_int(float x) {
    const float f = floorf(x);
    return f >= -2147483648.0f && f < 2147483648.0f ? (int)f : (-2147483647 - 1);
}

// model_utils.py:94-147: the four corner offsets into one [H, W] map (indices clamped to the map) and the four weights
// (from the unclamped corners).  Computed once per point; bilinear_blend applies them to as many maps as the point has channels.
struct BilinearTaps {
    long long i00, i01, i10, i11;
    float w00, w01, w10, w11;
};

__device__ __forceinline__ BilinearTaps bilinear_taps(int H, int W, float x, float y) {
#pragma clang fp contract(off)
    const int x0 = floor_int(x), y0 = floor_int(y);
    const long long x1 = (long long)x0 + 1, y1 = (long long)y0 + 1;
    const float x0f = (float)x0, x1f = (float)x1, y0f = (float)y0, y1f = (float)y1;
    const long long mx = W - 1, my = H - 1;
    const long long cx0 = x0 < 0 ? 0 : (x0 > mx ? mx : x0), cx1 = x1 < 0 ? 0 : (x1 > mx ? mx : x1);
    const long long cy0 = y0 < 0 ? 0 : (y0 > my ? my : y0), cy1 = y1 < 0 ? 0 : (y1 > my ? my : y1);
    BilinearTaps t;
    t.i00 = cy0 * W + cx0; t.i01 = cy0 * W + cx1; t.i10 = cy1 * W + cx0; t.i11 = cy1 * W + cx1;
    t.w00 = (x1f - x) * (y1f - y); t.w01 = (x - x0f) * (y1f - y); t.w10 = (x1f - x) * (y - y0f); t.w11 = (x - x0f) * (y - y0f);
    return t;
}

// model_utils.py:152-154 on one map: every product rounded, the sum left to right
__device__ __forceinline__ float bilinear_blend(const float *im, const BilinearTaps &t) {
#pragma clang fp contract(off)
    return ((t.w00 * im[t.i00] + t.w01 * im[t.i01]) + t.w10 * im[t.i10]) + t.w11 * im[t.i11];
}

// model_utils.py:94-154 on one [H, W] map
__device__ __forceinline__ float bilinear_clamped(const float *im, int H, int W, float x, float y) {
    return bilinear_blend(im, bilinear_taps(H, W, x, y));
}

}  // namespace bt
