// sample_taps.hpp — the two pieces of sampling arithmetic that more than one kernel must reproduce bit for bit, one copy each:
//   blend4            the reference's patchify blend (backend/altcorr/correlation.py:55-66): the four weights from the
//                     fractional offsets, every product rounded, the sum left to right.       k_patchify<true>, k_patch_generate
//   bilinear_clamped  bilinear_sample2d (frontend/core/model_utils.py:75-158) of one map: floor, indices clamped to the
//                     map, weights from the unclamped corners, the sum left to right.        k_observe_query, k_patch_generate
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

// model_utils.py:94-154 on one [H, W] map
__device__ __forceinline__ float bilinear_clamped(const float *im, int H, int W, float x, float y) {
#pragma clang fp contract(off)
    const int x0 = floor_int(x), y0 = floor_int(y);
    const long long x1 = (long long)x0 + 1, y1 = (long long)y0 + 1;
    const float x0f = (float)x0, x1f = (float)x1, y0f = (float)y0, y1f = (float)y1;
    const long long mx = W - 1, my = H - 1;
    const long long cx0 = x0 < 0 ? 0 : (x0 > mx ? mx : x0), cx1 = x1 < 0 ? 0 : (x1 > mx ? mx : x1);
    const long long cy0 = y0 < 0 ? 0 : (y0 > my ? my : y0), cy1 = y1 < 0 ? 0 : (y1 > my ? my : y1);
    const float i00 = im[cy0 * W + cx0], i01 = im[cy0 * W + cx1], i10 = im[cy1 * W + cx0], i11 = im[cy1 * W + cx1];
    const float w00 = (x1f - x) * (y1f - y), w01 = (x - x0f) * (y1f - y), w10 = (x1f - x) * (y - y0f), w11 = (x - x0f) * (y - y0f);
    return ((w00 * i00 + w01 * i01) + w10 * i10) + w11 * i11;                  // model_utils.py:152-154, left to right
}

}  // namespace bt
