// ba_update.hpp — what the kernels that end a step share (k_update / k_tile, ba_tile.hip; k_etile, ba_etile.hip; k_stream,
// k_edge2u, k_loose_update; k_solve_update, ba_solve_update.hpp): a track's new disparity and its clamp (ba.py:328, :333), the
// walk over a tile's slots one slot ahead, dX as tagged granules, the pose retraction Exp(dX) * G (groups.py:153-156) and the
// copy + clamp of the patch buffer.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_kernels.hpp"

namespace bt {

constexpr int kUpdGeo = 28;          // floats per pair in the LDS of an update's tile block: the 20 of kPairGeomFloats, delta (6), padding to 16 bytes

// ba.py:333.  Two selects, not fminf / fmaxf: a NaN disparity passes through, as it does in the reference.
__device__ __forceinline__ float clamp_disp(float dd) {
    dd = dd < 1e-3f ? 1e-3f : dd;
    return dd > 10.0f ? 10.0f : dd;
}
// a track's new disparity, dZ = Q (w' - tot) applied and clamped (ba.py:328, :333); tot = sum of its edges' Jz^T W Jj delta,
// 0 on a structure-only step (ba.py:316-317).  In R up to the rounding to float32.
template <typename R>
__device__ __forceinline__ float new_disp(R pdisp, R Q, R wp, R tot) { return clamp_disp((float)(pdisp + Q * (wp - tot))); }

// The slots [s0, s1) of a k_tile-layout tile that wave `wave` of `waves` walks
__device__ __forceinline__ void wave_slots(int nslot, int wave, int waves, int &s0, int &s1) {
    const int chunk = (nslot + waves - 1) / waves;
    s0 = wave * chunk; s1 = min(nslot, s0 + chunk);
}
// A lane's walk over such slots, fetched one slot ahead: the slot's edge (-1: none), local pair, target and weights.
// start() requests the first slot's table entries and fetch() its operands — apart, so that the caller can put work that
// needs neither between the two dependent trips to memory; advance() makes the fetched slot current and, if there is one,
// fetches slot `next`.
template <typename R>
struct SlotStream {
    int e = -1, lp = 0, e_nx = -1, lp_nx = 0;
    R tu = 0, tv = 0, w0 = 0, w1 = 0, tu_nx = 0, tv_nx = 0, w0_nx = 0, w1_nx = 0;
    __device__ __forceinline__ void start(const PlanDev &pd, int slot, int lane) {
        const size_t idx = (size_t)slot * kLanes + lane;
        e_nx = pd.slot_edge[idx]; lp_nx = pd.slot_lp[idx];
    }
    __device__ __forceinline__ void fetch(const StepArgs &a) {
        tu_nx = tv_nx = w0_nx = w1_nx = (R)0;
        if (e_nx >= 0) {
            const float *tp = a.targets + (size_t)e_nx * a.tstride;
            tu_nx = tp[0]; tv_nx = tp[1];
            const float2 w = reinterpret_cast<const float2 *>(a.weights)[e_nx];
            w0_nx = w.x; w1_nx = w.y;
        }
    }
    __device__ __forceinline__ void advance(const PlanDev &pd, const StepArgs &a, int next, bool more, int lane) {
        e = e_nx; lp = lp_nx; tu = tu_nx; tv = tv_nx; w0 = w0_nx; w1 = w1_nx;
        if (more) { start(pd, next, lane); fetch(a); }
    }
};

// dX as tagged granules (StepArgs::dxg; the fused solve + update launch, ba_solve_update.hpp): one 8-byte word per component,
// {float dx, uint32 tag}, written and read whole by relaxed agent-scope atomics.  The tag travels with the value, so the
// hand-off needs no fence and no separate flag; k_pair_finalize clears the tags every step, the solver publishes tag 1.
__device__ __forceinline__ void dx_publish(const StepArgs &a, int k, float v) {
    __hip_atomic_store(a.dxg + k, (unsigned long long)__float_as_uint(v) | (1ull << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one look at granule k: true, and its value, once it carries this step's tag
__device__ __forceinline__ bool dx_peek(const StepArgs &a, int k, float &v) {
    const unsigned long long g = __hip_atomic_load(a.dxg + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v = __uint_as_float((unsigned)g);
    return (unsigned)(g >> 32) == 1u;
}

__device__ inline void retract_pose(const float *pin, const float *xi, float *pout) {
    // poses' = Exp(xi) * G  (groups.py:153-156; so3.h:153-190; se3.h:134-142), in double
    const double tau[3] = {xi[0], xi[1], xi[2]}, phi[3] = {xi[3], xi[4], xi[5]};
    const double th2 = phi[0]*phi[0] + phi[1]*phi[1] + phi[2]*phi[2], th = sqrt(th2);
    double imag, real, c1, c2;
    if (th < 1e-6) {
        const double th4 = th2 * th2;
        imag = 0.5 - th2 / 48.0 + th4 / 3840.0;
        real = 1.0 - th2 / 8.0 + th4 / 384.0;
        c1 = 0.5 - th2 / 24.0;
        c2 = 1.0 / 6.0 - th2 / 120.0;
    } else {
        imag = sin(0.5 * th) / th;
        real = cos(0.5 * th);
        c1 = (1.0 - cos(th)) / th2;
        c2 = (th - sin(th)) / (th2 * th);
    }
    double qe[4] = {imag * phi[0], imag * phi[1], imag * phi[2], real};
    double nq = 1.0 / sqrt(qe[0]*qe[0] + qe[1]*qe[1] + qe[2]*qe[2] + qe[3]*qe[3]);
    for (int c = 0; c < 4; ++c) qe[c] *= nq;
    const double pxt[3] = {phi[1]*tau[2] - phi[2]*tau[1], phi[2]*tau[0] - phi[0]*tau[2], phi[0]*tau[1] - phi[1]*tau[0]};
    const double ppt[3] = {phi[1]*pxt[2] - phi[2]*pxt[1], phi[2]*pxt[0] - phi[0]*pxt[2], phi[0]*pxt[1] - phi[1]*pxt[0]};
    double te[3];
    for (int c = 0; c < 3; ++c) te[c] = tau[c] + c1 * pxt[c] + c2 * ppt[c];
    double q[4] = {pin[3], pin[4], pin[5], pin[6]};
    nq = 1.0 / sqrt(q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3]);
    for (int c = 0; c < 4; ++c) q[c] *= nq;
    const double t[3] = {pin[0], pin[1], pin[2]};
    double qo[4] = { qe[3]*q[0] + qe[0]*q[3] + qe[1]*q[2] - qe[2]*q[1],
                     qe[3]*q[1] - qe[0]*q[2] + qe[1]*q[3] + qe[2]*q[0],
                     qe[3]*q[2] + qe[0]*q[1] - qe[1]*q[0] + qe[2]*q[3],
                     qe[3]*q[3] - qe[0]*q[0] - qe[1]*q[1] - qe[2]*q[2] };
    nq = 1.0 / sqrt(qo[0]*qo[0] + qo[1]*qo[1] + qo[2]*qo[2] + qo[3]*qo[3]);
    double ux = qe[1]*t[2] - qe[2]*t[1], uy = qe[2]*t[0] - qe[0]*t[2], uz = qe[0]*t[1] - qe[1]*t[0];
    ux += ux; uy += uy; uz += uz;
    pout[0] = (float)(te[0] + t[0] + qe[3]*ux + (qe[1]*uz - qe[2]*uy));
    pout[1] = (float)(te[1] + t[1] + qe[3]*uy + (qe[2]*ux - qe[0]*uz));
    pout[2] = (float)(te[2] + t[2] + qe[3]*uz + (qe[0]*uy - qe[1]*ux));
    for (int c = 0; c < 4; ++c) pout[3 + c] = (float)(qo[c] * nq);
}

// patch `gid` < p_tot of the buffer is copied and clamped (ba.py:333; TRACKS_ELSEWHERE: patches that carry a track are
// written by the tile blocks and skipped here, else — the unfused structure-only update — their dZ = Q w' is applied here,
// ba.py:316-317), then one thread per buffer pose: Exp(dX) * G in double (groups.py:153-156) or, structure-only, a plain copy.
template <bool SO, bool TRACKS_ELSEWHERE>
__device__ __forceinline__ void update_rest(const PlanDev &pd, const StepArgs &a, int gid, int do_poses) {
    if (gid < pd.p_tot) {
        // track of this patch, or -1: bitmap + rank (most of the buffer's patches are not in the window)
        const unsigned aw = pd.act_bits[gid >> 5], ab = (unsigned)gid & 31u;
        const bool has = (aw >> ab) & 1u;
        if (TRACKS_ELSEWHERE && has) return;                            // written by its tile's block
        const float x = a.patches[3*gid], y = a.patches[3*gid + 1], d = a.patches[3*gid + 2];
        float dd = d;                                                   // ba.py:333 (whole buffer)
        if (SO && has) {                                                // ba.py:316-317
            const int trk = pd.act_rank[gid >> 5] + __popc(aw & ((1u << ab) - 1u));
            if (a.prec) { const double2 qw = reinterpret_cast<const double2 *>(a.qw)[trk]; dd = (float)((double)d + qw.x * qw.y); }
            else { const float2 qw = a.qw[trk]; dd = d + qw.x * qw.y; }
        }
        // (clamp_disp alone, not new_disp: a patch without a track has no (Q, w') to load)
        a.patches_out[3*gid] = x; a.patches_out[3*gid + 1] = y; a.patches_out[3*gid + 2] = clamp_disp(dd);
    } else if (do_poses && gid < pd.p_tot + pd.n_buf) {
        const int p = gid - pd.p_tot;
        if (SO) {
            for (int c = 0; c < 7; ++c) a.poses_out[7*p + c] = a.poses[7*p + c];
        } else {
            float xi[6] = {0, 0, 0, 0, 0, 0};
            if (p >= pd.fixedp && p < pd.fixedp + pd.n)
                for (int c = 0; c < 6; ++c) xi[c] = a.dx[6 * (p - pd.fixedp) + c];
            retract_pose(a.poses + 7*p, xi, a.poses_out + 7*p);
        }
    }
}

}  // namespace bt
