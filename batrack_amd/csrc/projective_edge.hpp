// projective_edge.hpp — the per-edge arithmetic of the fused reprojection, one copy for k_reproject
// (projective_kernels.hip) and the keyframe decision (keyframe.hip): iproj -> G_j * G_i^-1 -> act4 -> proj for one patch pixel.
// Formulas: the reference's main/backend/projective_ops.py:19-75, lietorch/include/se3.h:36-56, so3.h:31-60.
#pragma once
#include <hip/hip_runtime.h>

namespace bt {

struct Q4 { float x, y, z, w; };

__device__ __forceinline__ Q4 q_unit(Q4 q) {                                   // so3.h:35-37
    const float n = 1.0f / sqrtf(q.x*q.x + q.y*q.y + q.z*q.z + q.w*q.w);
    return {q.x*n, q.y*n, q.z*n, q.w*n};
}
__device__ __forceinline__ Q4 q_mul(Q4 a, Q4 b) {
    return { a.w*b.x + a.x*b.w + a.y*b.z - a.z*b.y,
             a.w*b.y - a.x*b.z + a.y*b.w + a.z*b.x,
             a.w*b.z + a.x*b.y - a.y*b.x + a.z*b.w,
             a.w*b.w - a.x*b.x - a.y*b.y - a.z*b.z };
}
__device__ __forceinline__ void q_rot(Q4 q, const float *p, float *o) {       // so3.h:55-60
    float ux = q.y*p[2] - q.z*p[1], uy = q.z*p[0] - q.x*p[2], uz = q.x*p[1] - q.y*p[0];
    ux += ux; uy += uy; uz += uz;
    o[0] = p[0] + q.w*ux + (q.y*uz - q.z*uy);
    o[1] = p[1] + q.w*uy + (q.z*ux - q.x*uz);
    o[2] = p[2] + q.w*uz + (q.x*uy - q.y*ux);
}

// One pixel `pat` (planes x, y, inverse depth `pe` floats apart) of a patch of frame i (pose pi, intrinsics Ki) into frame
// j (pj, Kj): out = (u, v[, projected inverse depth]); returns Z before the clamp.  G_i * G_i^-1 is computed as such when
// pi == pj: it is not replaced by the identity.
template <bool DEPTH, bool TONLY>
__device__ __forceinline__ float reproject_pixel(const float *pi, const float *pj, const float *Ki, const float *Kj,
                                                 const float *pat, int pe, float *out) {
    // X0 = ((x - cx)/fx, (y - cy)/fy, 1, d)                                           projective_ops.py:19-29
    const float d = pat[2 * pe];
    const float X0[3] = { (pat[0] - Ki[2]) / Ki[0], (pat[pe] - Ki[3]) / Ki[1], 1.0f };
    // Gij = G_j * G_i^-1                                                               se3.h:36-47
    const Q4 qi = q_unit({pi[3], pi[4], pi[5], pi[6]}), qj = q_unit({pj[3], pj[4], pj[5], pj[6]});
    const Q4 qiv = {-qi.x, -qi.y, -qi.z, qi.w};
    const float ti[3] = {pi[0], pi[1], pi[2]};
    float tiv[3], tr[3];
    q_rot(qiv, ti, tiv);
    tiv[0] = -tiv[0]; tiv[1] = -tiv[1]; tiv[2] = -tiv[2];
    q_rot(qj, tiv, tr);
    const float tij[3] = { pj[0] + tr[0], pj[1] + tr[1], pj[2] + tr[2] };
    float R[3];
    if (TONLY) { R[0] = X0[0]; R[1] = X0[1]; R[2] = X0[2]; }                           // projective_ops.py:61-64
    else q_rot(q_unit(q_mul(qj, qiv)), X0, R);
    // X1 = (R X0 + t d, d)                                                              se3.h:53-56
    const float X = R[0] + tij[0] * d, Y = R[1] + tij[1] * d, Z = R[2] + tij[2] * d;
    const float iz = 1.0f / fmaxf(Z, 1e-2f);                                            // projective_ops.py:43
    out[0] = Kj[0] * (iz * X) + Kj[2];
    out[1] = Kj[1] * (iz * Y) + Kj[3];
    if (DEPTH) out[2] = iz * d;
    return Z;
}

}  // namespace bt
