// ba_kernels.hip — gfx950 (CDNA4, wave64) kernels of the BA step.
//
// One BA_rgbd_droid call (/root/reference/main/backend/ba.py:217-339) becomes four launches
//   k_tile           one workgroup of 8 (16) waves per tile of up to 64 tracks: relative pose of
//                    the tile's camera pairs (Gij is per PAIR, not per edge: projective_ops.py:61),
//                    per-edge reprojection, Jacobians, robust weights (projective_ops.py:54-100,
//                    ba.py:228-266), per-track C / w / E, per-pair J^T W J, and the tile's Schur
//                    product E Q E^T on the f64 MFMA (ba.py:284-323)
//   k_pair_finalize  B and v of ba.py:279-290 from the per-pair sums
//   k_solve_*        damped block-sparse Cholesky of the reduced camera system in LDS, forward and
//                    back substitution (ba.py:60-70,323-325): k_solve_pipe (barrier-free sweep) where
//                    the plan allows it, else k_solve_fused / k_solve_lds / k_solve_global
//   k_update         back-substitution of the depths, clamp of the whole buffer, pose retraction
//                    (ba.py:328-337, groups.py:153-156); leaves [S | y] clear for the next step
// plus k_pack_system for the multi-GPU exchange form.  A structure-only call is k_tile<SO> + k_update<SO>.
//
// Algebra used throughout: Ji = -Jj * Ad(Gij), so with
// per-pair sums  Bjj = sum Jj^T W Jj,  gj = sum Jj^T W r  the blocks are
//   B[a,a] += Ad^T Bjj Ad   B[b,a] += -Bjj Ad   B[b,b] += Bjj
//   v[a]   += -Ad^T gj      v[b]   += gj        E[a,k] += -Ad^T Ej   E[b,k] += Ej
// and Ji is never formed per edge.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdlib>
#include <utility>

#include "ba_kernels.hpp"
#include "probe.hpp"
#include "ba_edge.hpp"
#include "ba_update.hpp"
#include "dev_cache.hpp"

namespace bt {

__device__ __forceinline__ double dpp_add8(double v);     // (defined with the solver's helpers below)

// ------------------------------------------------------------------ k_tile
// One workgroup of 8 waves per tile of <= 64 tracks; lane l of every wave owns track l.
// Wave w takes a contiguous chunk of the tile's edge slots (one slot each on the
// regular 8-observation graphs), so a wave sees one camera pair per slot and the
// per-pair sums are full-wave reductions.
// LDS: Eh[R16][66]   local E: row = 6*local_cam + comp, column = lane = track
//      stg[8][8][64] per-wave partials of (E at the source camera, C, w) per track
//      las[8][64]    local source camera of those partials
//      Qs[128] (Q, then beta = Q w' per track), gidx[R16] (global row of a local row), geo[pairs][20]
// E accumulation never uses LDS atomics on the common path: a track's target-camera
// rows are written by the wave that owns the slot (plain read-add-write), its
// source-camera row is summed in registers and merged by an owner thread after the
// barrier.  Only a duplicated (track, target camera) observation that straddles two
// waves' slot ranges falls back to ds_add_f32, and the plan cuts the ranges where no such run crosses if it can.
// One tile per workgroup (graphs of up to a few thousand tiles, e.g. the 64-KF / 131k-edge benchmark and the
// sliding-window graphs; larger ones take k_edge2 / k_stream): no cross-tile state, Schur tiles go straight from
// the MFMA registers to the atomics.
// WIDE: 16 waves per tile instead of 8, for graphs of few tiles with deep slot loops (a sliding window of 50 frames:
// 40 tiles of 54 slots): the tile's latency, which is all there is on a quarter-empty GPU, shrinks with the chunk.
// The part of a step's last kernel that is not per tile: patch `gid` < p_tot of the buffer is copied and clamped (ba.py:333;
// TRACKS_ELSEWHERE: patches that carry a track are written by the tile blocks and skipped here, else — the unfused
// structure-only update — their dZ = Q w' is applied here, ba.py:316-317), then one thread per buffer pose: Exp(dX) * G in
// double (groups.py:153-156) or, structure-only, a plain copy.
// FUSE (structure-only steps): the workgroups behind the pd.T tile workgroups do update_rest, and every tile writes its
// tracks' new disparities itself: the whole structure-only step is ONE launch instead of k_tile<SO> + k_update<SO>.
// R: float or double — the precision of the per-edge maths, of E in LDS and of the (Q, w') it leaves for k_update (float64 is
// the default of this kernel: StepArgs::prec).  The float64 variant is allowed 256 registers (two 8-wave tiles per CU).
template <bool SO, bool PROF, bool WIDE = false, bool FUSE = false, typename R = float>
#ifndef BT_TILE64_WAVES
#define BT_TILE64_WAVES 2
#endif
__global__ __launch_bounds__(WIDE ? 1024 : 512, WIDE ? 2 : (sizeof(R) == 8 ? BT_TILE64_WAVES : 4)) void k_tile(PlanDev pd, StepArgs a, int do_poses) {
    if (FUSE && (int)blockIdx.x >= pd.T) {
        update_rest<true, true>(pd, a, ((int)blockIdx.x - pd.T) * (int)blockDim.x + (int)threadIdx.x, do_poses);
        return;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    R *lds = reinterpret_cast<R *>(lds_raw);
    typedef typename Vec2<R>::type R2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nthr = blockDim.x, kTileWaves = nthr >> 6;          // 8 or 16 waves per tile (launch parameter)
    long long pf[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tc = PROF ? clock64() : 0, tn;
#define BT_PF(i) do { if (PROF) { __builtin_amdgcn_sched_barrier(0); tn = clock64(); pf[i] += tn - tc; tc = tn; __builtin_amdgcn_sched_barrier(0); } } while (0)
    BT_PROBE_TILE_DECL();         // (measurement hooks: probe.hpp, tools/probes/wave_times.hpp)
#define BT_WT(i) BT_PROBE_TILE_MARK(i)
    // LDS carve-up for the largest tile of the plan (fixed offsets: tiles of one workgroup differ in size)
    const int R16max = SO ? 0 : pd.max_rows16;
    R *Eh = lds, *stg = Eh + R16max * kLdsRowStride;
    R *Qs = stg + kTileWaves * 8 * 64;                            // (Qs: Q of the 64 tracks, then beta = Q w')
    R *geo = Qs + 128;                                            // [npair][20], 16-byte aligned
    int *las = reinterpret_cast<int *>(geo + (size_t)(pd.max_tile_pairs > 0 ? pd.max_tile_pairs : 1) * kPairGeomFloats);
    int *gidx = las + kTileWaves * 64;
    // one per-pair sum per wave in registers
    double pacc = 0.0;
    int p_cur = -1;
    auto flush_pair = [&]() {
        const int vi = (lane >> 1) & 31;
        if (p_cur >= 0 && (lane & 1) == 0 && vi < 27)
            atomicAdd(&a.pairacc[(size_t)p_cur * kPairAccStride + vi], pacc);
        pacc = 0.0; p_cur = -1;
    };
    // Workgroups are dealt round-robin to the 8 XCDs (each with its own L2): XCD x gets workgroups x, x + 8, ...  Give it a
    // CONTIGUOUS range of tiles instead — the tiles of one source frame are neighbours and share cameras, pair geometry and
    // the rows of S they add to (1024 tiles: 38.9 -> 32.7 us; nothing at 256 tiles, where every CU holds one workgroup).
    const int tq_ = pd.T >> 3, tr_ = pd.T & 7, xcd_ = blockIdx.x & 7;
    const int tile_begin = xcd_ * tq_ + min(xcd_, tr_) + (blockIdx.x >> 3), tile_end = tile_begin + 1;
#pragma unroll 1
    for (int tile = tile_begin; tile < tile_end; ++tile) {
        const int ntrk = pd.tile_ntrk[tile], ncam = pd.tile_ncam[tile];
        const int Rw = 6 * ncam, R16 = SO ? 0 : ((Rw + 15) >> 4) << 4;
        const int *cams = pd.tile_cams + pd.tile_cam0[tile];
        if (!SO) {                                                 // local row -> row of the reduced system
            for (int i = tid; i < R16max; i += nthr) gidx[i] = i < Rw ? 6 * cams[i / 6] + i % 6 : -1;
        }
        // first loads that need nothing but the tile index: the cameras of its pairs and the patch of this lane's track
        const int mtp = pd.max_tile_pairs > 0 ? pd.max_tile_pairs : 1;
        const int ij0 = tid < mtp ? pd.tile_ij[(size_t)tile * mtp + tid] : 0;
        const int patch_ld = pd.tile_kx[(size_t)tile * kLanes + lane];
        const int slot0 = pd.tile_slot0[tile], nslot = pd.tile_nslot[tile];
        // this wave's slots: the plan's cuts (at boundaries that no run of repeated observations crosses, ba_plan.cpp)
        const uint16_t *cut = WIDE ? pd.tile_cut16 + (size_t)tile * 17 : pd.tile_cut8 + (size_t)tile * 9;
        const int s0 = cut[wave], s1 = cut[wave + 1];
        // this wave's first slot, in flight while the pair geometry is computed
        int e_nx = -1, pair_nx = 0, lp_nx = 0;
        unsigned lab_nx = 0xffffu;
        if (s0 < s1) {
            const size_t idx = (size_t)(slot0 + s0) * kLanes + lane;
            e_nx = pd.slot_edge[idx]; pair_nx = pd.slot_pair[idx]; lab_nx = pd.slot_lab[idx]; lp_nx = pd.slot_lp[idx];
        }
        {                                                          // relative pose of the tile's camera pairs
            const int np = pd.tile_npair[tile];
            // (the pair's global index: only to leave the result for k_pair_finalize, which then need not redo it)
            const int gp0 = !SO && tid < np ? pd.tile_pairs[pd.tile_pair0[tile] + tid] : 0;
            for (int p = tid; p < np; p += nthr) {                 // (more pairs than threads: never with kMaxTilePairs = 192)
                const int ij = p == tid ? ij0 : pd.tile_ij[(size_t)tile * mtp + p];
                R *g = geo + p * kPairGeomFloats;
                pair_geometry<R>(a.poses, a.intr, ij & 0xffff, ij >> 16, g);
                if (!SO) {
                    const int gp = p == tid ? gp0 : pd.tile_pairs[pd.tile_pair0[tile] + p];
                    R2 *dst = reinterpret_cast<R2 *>(reinterpret_cast<R *>(a.pairgeo) + (size_t)gp * kPairGeomFloats);
                    const R2 *src = reinterpret_cast<const R2 *>(g);
#pragma unroll
                    for (int c = 0; c < kPairGeomFloats / 2; ++c) dst[c] = src[c];
                }
            }
        }
        for (int i = tid; i < R16 * kLdsRowStride; i += nthr) Eh[i] = (R)0;

        const int trk = pd.tile_trk0[tile] + lane;
        const bool has_trk = lane < ntrk;
        int patch = 0;
        R px = 0, py = 0, pdisp = 0;
        R mono_v = 0;
        if (has_trk) {
            patch = patch_ld;
            px = a.patches[3*patch]; py = a.patches[3*patch + 1]; pdisp = a.patches[3*patch + 2];
            mono_v = a.mono[(size_t)patch * a.mstride];                 // needed only after the slot loop: no load latency there
        }
        R tu_nx = 0, tv_nx = 0, w0_nx = 0, w1_nx = 0;
        if (e_nx >= 0) {
            const float *tp = a.targets + (size_t)e_nx * a.tstride;
            tu_nx = tp[0]; tv_nx = tp[1];
            const float2 w = reinterpret_cast<const float2 *>(a.weights)[e_nx];
            w0_nx = w.x; w1_nx = w.y;
        }
        __syncthreads();
        BT_PF(0);
        BT_WT(1);

        R Cacc = 0, wacc = 0, Ei[6] = {0, 0, 0, 0, 0, 0};
        unsigned la_cur = 0xffu;
        // Target cameras this track also observes in the neighbouring waves' chunks right across the
        // chunk boundary.  Observations of one (track, camera) are contiguous in slot order, so a run
        // that continues into a neighbour's chunk is recognised by these two values; every slot of
        // such a run must use LDS atomics (the neighbour updates the same element concurrently).
        unsigned lb_prev = 0xffu, lb_next = 0xffu;
        if (!SO && s0 < s1) {
            if (s0 > 0) lb_prev = pd.slot_lab[(size_t)(slot0 + s0 - 1) * kLanes + lane] >> 8;
            if (s1 < nslot) lb_next = pd.slot_lab[(size_t)(slot0 + s1) * kLanes + lane] >> 8;
        }
        R Ejacc[6] = {0, 0, 0, 0, 0, 0};
        unsigned lb_acc = 0xffu;
        auto flush_ej = [&](unsigned lbf) {
            if (lbf != 0xffu) {
                R *row = Eh + lbf * 6 * kLdsRowStride + lane;
                if (lbf == lb_prev || lbf == lb_next) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) atomicAdd(row + c * kLdsRowStride, Ejacc[c]);
                } else {
#pragma unroll
                    for (int c = 0; c < 6; ++c) row[c * kLdsRowStride] += Ejacc[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) Ejacc[c] = (R)0;
        };
#pragma unroll 1
        for (int s = s0; s < s1; ++s) {
            const size_t idx = (size_t)(slot0 + s) * kLanes + lane;
            // this slot's operands were loaded one iteration ahead (the first one before the barrier above)
            const int e = e_nx, pair = pair_nx, lp = lp_nx;
            const bool act = e >= 0;
            const unsigned lab = lab_nx;
            const R tu = tu_nx, tv = tv_nx, w0 = w0_nx, w1 = w1_nx;
            if (s + 1 < s1) {
                const size_t idn = idx + kLanes;
                e_nx = pd.slot_edge[idn]; pair_nx = pd.slot_pair[idn]; lab_nx = pd.slot_lab[idn]; lp_nx = pd.slot_lp[idn];
                tu_nx = tv_nx = w0_nx = w1_nx = (R)0;
                if (e_nx >= 0) {
                    const float *tp = a.targets + (size_t)e_nx * a.tstride;
                    tu_nx = tp[0]; tv_nx = tp[1];
                    const float2 w = reinterpret_cast<const float2 *>(a.weights)[e_nx];
                    w0_nx = w.x; w1_nx = w.y;
                }
            }
            R g[kPairGeomFloats];
            if (sizeof(R) == 4) {
                const float4 *g4 = reinterpret_cast<const float4 *>(geo + (size_t)lp * kPairGeomFloats);
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    const float4 t4 = g4[c];
                    g[4*c] = t4.x; g[4*c + 1] = t4.y; g[4*c + 2] = t4.z; g[4*c + 3] = t4.w;
                }
            } else {
                const double2 *g2 = reinterpret_cast<const double2 *>(geo + (size_t)lp * kPairGeomFloats);
#pragma unroll
                for (int c = 0; c < 10; ++c) { const double2 t2 = g2[c]; g[2*c] = t2.x; g[2*c + 1] = t2.y; }
            }
            if (PROF) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
            BT_PF(1);
            EdgeQT<R> q;
            edge_eval<R>(g, px, py, pdisp, tu, tv, w0, w1, a, q);
            if (!act) { q.W0 = (R)0; q.W1 = (R)0; q.r0 = (R)0; q.r1 = (R)0; }

            // C, w of the track (ba.py:287,292)
            Cacc += q.W0 * q.jz0 * q.jz0 + q.W1 * q.jz1 * q.jz1;
            wacc += q.W0 * q.jz0 * q.r0 + q.W1 * q.jz1 * q.r1;
            if (SO) continue;

            const R wa0 = q.W0 * q.a0, wa2 = q.W0 * q.a2, wa3 = q.W0 * q.a3, wa4 = q.W0 * q.a4, wa5 = q.W0 * q.a5;
            const R wb1 = q.W1 * q.b1, wb2 = q.W1 * q.b2, wb3 = q.W1 * q.b3, wb4 = q.W1 * q.b4, wb5 = q.W1 * q.b5;
            // Ej = Jj^T W Jz (ba.py:263) and Ei = -Ad^T Ej
            const R Ej[6] = { wa0 * q.jz0, wb1 * q.jz1, fma_t(wa2, q.jz0, wb2 * q.jz1), fma_t(wa3, q.jz0, wb3 * q.jz1),
                              fma_t(wa4, q.jz0, wb4 * q.jz1), fma_t(wa5, q.jz0, wb5 * q.jz1) };
            const unsigned la = lab & 0xffu, lb = lab >> 8;
            // target-camera E: repeated observations of one (track, camera) are consecutive slots, so they
            // are summed in registers and written once when the camera changes (or the chunk ends)
            if (act && lb != lb_acc) {
                flush_ej(lb_acc);
                lb_acc = lb;
            }
            if (act && lb != 0xffu) {
#pragma unroll
                for (int c = 0; c < 6; ++c) Ejacc[c] += Ej[c];
            }
            if (act && la != 0xffu) {
                la_cur = la;                 // one source camera per track: enforced by the plan (ii = ix[kk], batrack.py:199)
                // o_tau = R^T e_tau ; o_phi = R^T (e_tau x t + e_phi)      (se3.h:58-67)
                const R cx = Ej[1]*g[11] - Ej[2]*g[10] + Ej[3];
                const R cy = Ej[2]*g[9]  - Ej[0]*g[11] + Ej[4];
                const R cz = Ej[0]*g[10] - Ej[1]*g[9]  + Ej[5];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    Ei[c]     -= g[c]*Ej[0] + g[3 + c]*Ej[1] + g[6 + c]*Ej[2];
                    Ei[3 + c] -= g[c]*cx + g[3 + c]*cy + g[6 + c]*cz;
                }
            }
            BT_PF(2);

            // per-pair sums: Bjj (21, row-major upper triangle) and gj (6)   (ba.py:260,266).  The 27
            // products are formed inside the loop (one pass per distinct pair of the slot, a single
            // pass on regular graphs) so that no second copy of them stays live.
            unsigned long long todo = __ballot(act);
            while (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const int p0 = __shfl(pair, leader);
                const R m = (act && pair == p0) ? (R)1 : (R)0;
                const R ma0 = m * wa0, mb1 = m * wb1, ma2 = m * wa2, mb2 = m * wb2, ma3 = m * wa3, mb3 = m * wb3,
                            ma4 = m * wa4, mb4 = m * wb4, ma5 = m * wa5, mb5 = m * wb5;
                R v[32];
                v[0] = ma0 * q.a0;  v[1] = (R)0;        v[2] = ma0 * q.a2;  v[3] = ma0 * q.a3;
                v[4] = ma0 * q.a4;  v[5] = ma0 * q.a5;
                v[6] = mb1 * q.b1;  v[7] = mb1 * q.b2;  v[8] = mb1 * q.b3;  v[9] = mb1 * q.b4;  v[10] = mb1 * q.b5;
                v[11] = fma_t(ma2, q.a2, mb2 * q.b2); v[12] = fma_t(ma2, q.a3, mb2 * q.b3);
                v[13] = fma_t(ma2, q.a4, mb2 * q.b4); v[14] = fma_t(ma2, q.a5, mb2 * q.b5);
                v[15] = fma_t(ma3, q.a3, mb3 * q.b3); v[16] = fma_t(ma3, q.a4, mb3 * q.b4); v[17] = fma_t(ma3, q.a5, mb3 * q.b5);
                v[18] = fma_t(ma4, q.a4, mb4 * q.b4); v[19] = fma_t(ma4, q.a5, mb4 * q.b5);
                v[20] = fma_t(ma5, q.a5, mb5 * q.b5);
                v[21] = ma0 * q.r0; v[22] = mb1 * q.r1;
                v[23] = fma_t(ma2, q.r0, mb2 * q.r1); v[24] = fma_t(ma3, q.r0, mb3 * q.r1);
                v[25] = fma_t(ma4, q.r0, mb4 * q.r1); v[26] = fma_t(ma5, q.r0, mb5 * q.r1);
                v[27] = v[28] = v[29] = v[30] = v[31] = (R)0;
                wave_reduce_scatter32(v, lane);
                if (p0 != p_cur) { flush_pair(); p_cur = p0; }   // same pair as this wave's previous slot / tile: keep summing
                pacc += (double)v[0];
                todo &= ~__ballot(act && pair == p0);
            }
            BT_PF(3);
        }
        BT_WT(2);
        if (!SO) flush_ej(lb_acc);

        // per-wave partials -> LDS
#pragma unroll
        for (int c = 0; c < 6; ++c) stg[(wave * 8 + c) * 64 + lane] = Ei[c];
        stg[(wave * 8 + 6) * 64 + lane] = Cacc;
        stg[(wave * 8 + 7) * 64 + lane] = wacc;
        las[wave * 64 + lane] = (int)la_cur;
        __syncthreads();
        if (!SO && wave < 6) {                          // owner of component `wave` of every track's source-camera E
            // a track has ONE source camera (plan-enforced), so the waves' partials of a lane all go to the same
            // element: all loads first, one read-modify-write
            R sum = 0;
            int la = 0xff;
            for (int w0 = 0; w0 < kTileWaves; w0 += 8) {
                int lw[8];
                R pv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const bool in = w0 + u < kTileWaves;
                    lw[u] = in ? las[(w0 + u) * 64 + lane] : 0xff;
                    pv[u] = in ? stg[((w0 + u) * 8 + wave) * 64 + lane] : (R)0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) if (lw[u] != 0xff) { sum += pv[u]; la = lw[u]; }
            }
            if (la != 0xff) Eh[(la * 6 + wave) * kLdsRowStride + lane] += sum;
        }
        if (wave == 6) {                                                   // ba.py:296-311
            R C = 0, wv = 0;
            for (int w = 0; w < kTileWaves; ++w) { C += stg[(w * 8 + 6) * 64 + lane]; wv += stg[(w * 8 + 7) * 64 + lane]; }
            R Q = 0, wp = 0;
            if (has_trk) {
                const R mono = mono_v;
                const R pm = mono > (R)1e-2f ? (R)1 : (R)0;               // (the prior is float32 data: compared as such)
                R Ca = C + pm * (R)a.alpha;
                Ca = Ca + (R)(a.lmbda_trk ? a.lmbda_trk[pd.trk_off + trk] : a.lmbda);
                wp = wv - pm * (R)a.alpha * (pdisp - mono);
                Q = sizeof(R) == 8 ? (R)frcp((double)Ca) : (R)1 / Ca;      // (float64: seed + two Newton steps, < 1e-15; the IEEE divide is ~30 instructions)
                if (FUSE) {                                                // ba.py:316-317, :333
                    float dd = (float)(pdisp + Q * wp);
                    dd = dd < 1e-3f ? 1e-3f : dd;
                    dd = dd > 10.0f ? 10.0f : dd;
                    a.patches_out[3*patch] = (float)px; a.patches_out[3*patch + 1] = (float)py; a.patches_out[3*patch + 2] = dd;
                } else {
                    R2 qw2; qw2.x = Q; qw2.y = wp;
                    reinterpret_cast<R2 *>(a.qw)[trk] = qw2;
                }
            }
            if (!SO) { Qs[lane] = Q; Qs[64 + lane] = Q * wp; }
        }
        __syncthreads();
        BT_PF(4);
        BT_WT(3);
        if (SO) continue;

        BT_PF(5);

        // Schur product of the tile on the matrix cores: out[i][j] += sum_k Q_k Eh[i][k] Eh[j][k] over the 64 tracks,
        // one 16x16 output tile per wave, on v_mfma_f64_16x16x4_f64: the float32 products are exact in double, so the sums
        // carry no float32 accumulation error (float32 partial sums were measured: no faster here — the tile's time is
        // its atomics — and 8x the dX error on the reference's ill-conditioned 8-frame case, for S and for y alike).
        // The wave of a diagonal tile has the rows of E it needs for E (Q w'), the Schur term of y (ba.py:311), in
        // registers: one more product with beta = Q w' in every column of B, column 0 of the result emitted.
        // E (Q w'), the Schur term of y (ba.py:311): every row of E against beta = Q w', eight threads per row on the vector
        // pipe, float64 (it used to be a second product of the diagonal tiles' waves on the matrix pipe: 16 more f64 MFMAs on
        // three of the eight waves — the tile's critical path at one tile per CU)
        for (int row = tid >> 3; row < Rw; row += nthr >> 3) {
            const int part = tid & 7;
            const R *er = Eh + row * kLdsRowStride + part;
            double s8 = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) s8 += (double)er[8 * k] * (double)Qs[64 + part + 8 * k];
            s8 = dpp_add8(s8);
            if (part == 0) atomicAdd(&a.y[gidx[row]], -s8);
        }
        const int nt = R16 >> 4, ntl = nt * (nt + 1) / 2;
        for (int t = wave; t < ntl; t += kTileWaves) {
            int ti = 0, base = 0;
            while (base + ti + 1 <= t) { base += ti + 1; ++ti; }
            const int tj = t - base;
            const int li = lane & 15, kq = lane >> 4;
            const R *ar = Eh + (16 * ti + li) * kLdsRowStride + kq;
            const R *br = Eh + (16 * tj + li) * kLdsRowStride + kq;
            const R *qr = Qs + kq;
            R av[16], bv[16], qv[16];
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) { av[ks] = ar[4 * ks]; bv[ks] = br[4 * ks]; qv[ks] = qr[4 * ks]; }
            double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < 16; ++ks)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[ks] * (double)qv[ks], (double)bv[ks], acc, 0, 0, 0);
            // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
            const int gc = gidx[16 * tj + li];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * ti + kq + 4 * r;
                if (gc >= 0 && row < Rw) { const int gr = gidx[row]; if (gr >= gc) atomicAdd(&a.S[(size_t)gr * pd.D + gc], -acc[r]); }
            }
        }
        BT_PF(6);
        BT_WT(4);
    }
    if (!SO) {
        flush_pair();
        BT_PF(7);
    }
    BT_PROBE_TILE_END(!SO && !FUSE, lane, wave, kTileWaves);
#undef BT_WT
    if (PROF && lane == 0 && wave == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x / 2)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        BT_PF(8);
        long long *o = reinterpret_cast<long long *>(a.status + 4) + (blockIdx.x == 0 ? 20 : 30);
        for (int i = 0; i < 10; ++i) o[i] = pf[i];
    }
#undef BT_PF
}

// ------------------------------------------------------------------ k_pair_finalize
// One wave per camera pair, in double.  sym index of (p<=q) in the 21-vector:
__device__ __forceinline__ int sym21(int p, int q) {
    if (p > q) { const int t = p; p = q; q = t; }
    return p * 6 - p * (p - 1) / 2 + (q - p);
}

// Blocks behind the pair blocks (plans with sp_ok, Jacobian kernel k_etile): per group of consecutive same-camera tiles, one
// block per 16x16 tile of the Schur product E Q E^T (its 256 threads one element each, summed over the group's tiles in
// tile order: independent loads, eight in flight) and one for E Q w'; subtracted from [S | y] — a few atomics per element
// and step instead of one per element and TILE.
__global__ __launch_bounds__(256) void k_pair_finalize(PlanDev pd, StepArgs a, int pair_blocks) {
    if ((int)blockIdx.x >= pair_blocks) {
        const int R16 = pd.max_rows16, nt = R16 >> 4, ntl = nt * (nt + 1) / 2;
        const int g = ((int)blockIdx.x - pair_blocks) / (ntl + 1), b = ((int)blockIdx.x - pair_blocks) - g * (ntl + 1);
        const size_t per_tile = sp_tile_doubles(pd.max_rows16, pd.max_tile_pairs);
        const int t0 = pd.sg_ptr[g], t1 = pd.sg_ptr[g + 1];
        const int *cams = pd.tile_cams + pd.tile_cam0[t0];           // the cameras of every tile of the group
        const int Rw = 6 * pd.tile_ncam[t0];
        auto grow = [&](int r) { return 6 * cams[r / 6] + r % 6; };
        auto group_sum = [&](const double *src) {
            double sum = 0.0;
            for (int t = t0; t < t1; t += 8) {
                double v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = t + k < t1 ? src[(size_t)(t + k) * per_tile] : 0.0;
#pragma unroll
                for (int k = 0; k < 8; ++k) sum += v[k];
            }
            return sum;
        };
        if (b < ntl) {
            int ti = 0, base = 0;
            while (base + ti + 1 <= b) { base += ti + 1; ++ti; }
            const int tj = b - base, j = threadIdx.x, r = j >> 6, lane = j & 63;
            const int row = 16 * ti + (lane >> 4) + 4 * r, col = 16 * tj + (lane & 15);
            if (row < Rw && col < Rw) {
                const int gr = grow(row), gc = grow(col);
                if (gr >= gc) atomicAdd(&a.S[(size_t)gr * pd.D + gc], -group_sum(a.spart + (size_t)b * 256 + j));
            }
        } else {
            for (int row = threadIdx.x; row < Rw; row += blockDim.x)
                atomicAdd(&a.y[grow(row)], -group_sum(a.spart + (size_t)ntl * 256 + row));
        }
        return;
    }
    __shared__ double sB[4][36], sAd[4][36], sM[4][36], sg[4][6];
    __shared__ double sgeo[4][kPairGeomFloats];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + w;
    if (a.priv) {
        // k_edge2's private copies of y (ba_plan.hpp: kPrivY): added up, cleared, and the sum added to y
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < pd.D; i += pair_blocks * blockDim.x) {
            double s = 0.0;
            for (int c = 0; c < kPrivY; c += 8) {
                double v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = a.priv[(size_t)(c + k) * pd.D + i];
#pragma unroll
                for (int k = 0; k < 8; ++k) { s += v[k]; if (v[k] != 0.0) a.priv[(size_t)(c + k) * pd.D + i] = 0.0; }
            }
            if (s != 0.0) atomicAdd(&a.y[i], s);
        }
        // ... and its arrival counters cleared for the next step
        int *arr = reinterpret_cast<int *>(a.priv + priv_copy_doubles((size_t)pd.D, (size_t)pd.P));
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kPrivArrive; i += pair_blocks * blockDim.x) if (arr[i] != 0) arr[i] = 0;
    }
    const bool live = p < pd.P;
    int ia = -1, ib = -1;
    if (live) {
        ia = pd.pair_i[p] - pd.fixedp; ib = pd.pair_j[p] - pd.fixedp;
        double *acc = a.pairacc + (size_t)p * kPairAccStride;
        double *g = sgeo[w];
        // the sums first (they need only the pair index), so their latency runs under the pose loads and the geometry
        double accv = 0.0;
        const int vi_ld = lane < 36 ? sym21(lane / 6, lane % 6) : lane < 42 ? 21 + lane - 36 : -1;
        if (pair_blocks < (int)gridDim.x) {
            // (k_etile left the tiles' sums side by side: added up here in the order of the plan's list — the list entries
            //  through the lanes, then independent loads, eight in flight)
            const int R16 = pd.max_rows16, nt = R16 >> 4;
            const size_t per_tile = sp_tile_doubles(pd.max_rows16, pd.max_tile_pairs), off = (size_t)nt * (nt + 1) / 2 * 256 + R16;
            const size_t mtp_s = (size_t)(pd.max_tile_pairs > 0 ? pd.max_tile_pairs : 1);
            const int q0 = pd.pp_ptr[p], q1 = pd.pp_ptr[p + 1];
            const double *src = a.spart + off + (size_t)(vi_ld >= 0 ? vi_ld : 0) * mtp_s;
            for (int qb = q0; qb < q1; qb += 64) {
                const int e_l = qb + lane < q1 ? pd.pp_idx[qb + lane] : 0, cnt = min(64, q1 - qb);
                for (int k0 = 0; k0 < cnt; k0 += 8) {
                    double v[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int e = __shfl(e_l, k0 + k);
                        v[k] = (k0 + k < cnt && vi_ld >= 0) ? src[(size_t)(e >> 6) * per_tile + (size_t)(e & 63)] : 0.0;      // [vi][pair] per tile
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) accv += v[k];
                }
            }
        } else if (vi_ld >= 0) {
            accv = acc[vi_ld];
            if (a.priv) {                     // ... and of the per-pair sums (kPrivP)
                double *pp = a.priv + (size_t)kPrivY * pd.D + (size_t)p * kPairAccStride + vi_ld;
                const size_t cs = (size_t)pd.P * kPairAccStride;
                double v[kPrivP];
#pragma unroll
                for (int c = 0; c < kPrivP; ++c) v[c] = pp[c * cs];
#pragma unroll
                for (int c = 0; c < kPrivP; ++c) accv += v[c];
            }
        }
        if (lane < kPairGeomFloats)                                                              // computed by the Jacobian kernel
            g[lane] = a.prec ? reinterpret_cast<const double *>(a.pairgeo)[(size_t)p * kPairGeomFloats + lane]
                             : (double)a.pairgeo[(size_t)p * kPairGeomFloats + lane];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (lane < 36) {
            const int r = lane / 6, c = lane % 6;
            sB[w][lane] = accv;
            // Ad = [[R, [t]x R], [0, R]]                                   (se3.h:58-67)
            double v = 0.0;
            if (r < 3 && c < 3) v = g[3*r + c];
            else if (r >= 3 && c >= 3) v = g[3*(r - 3) + (c - 3)];
            else if (r < 3 && c >= 3) {
                const int cc = c - 3;
                const double t0 = g[9], t1 = g[10], t2 = g[11];
                const double R0 = g[cc], R1 = g[3 + cc], R2 = g[6 + cc];
                v = r == 0 ? (-t2 * R1 + t1 * R2) : r == 1 ? (t2 * R0 - t0 * R2) : (-t1 * R0 + t0 * R1);
            }
            sAd[w][lane] = v;
        } else if (lane < 42) {
            sg[w][lane - 36] = accv;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (lane < 27 && pair_blocks == (int)gridDim.x) acc[lane] = 0.0;       // leave the per-pair sums clear for the next step
        if (a.priv && lane < 27 && pair_blocks == (int)gridDim.x) {
            double *pp = a.priv + (size_t)kPrivY * pd.D + (size_t)p * kPairAccStride + lane;
            const size_t cs = (size_t)pd.P * kPairAccStride;
#pragma unroll
            for (int c = 0; c < kPrivP; ++c) pp[c * cs] = 0.0;
        }
    }
    __syncthreads();
    if (live && lane < 36) {
        const int r = lane / 6, c = lane % 6;
        double m = 0.0;
        for (int s = 0; s < 6; ++s) m += sB[w][6*r + s] * sAd[w][6*s + c];
        sM[w][lane] = m;                                          // M = Bjj Ad
    }
    __syncthreads();
    if (!live) return;
    const int D = pd.D;
    if (lane < 36) {
        const int r = lane / 6, c = lane % 6;
        if (ia >= 0) {                                            // B[a,a] += Ad^T M
            double v = 0.0;
            for (int s = 0; s < 6; ++s) v += sAd[w][6*s + r] * sM[w][6*s + c];
            if (r >= c) atomicAdd(&a.S[(size_t)(6*ia + r) * D + 6*ia + c], v);
        }
        if (ib >= 0 && r >= c) atomicAdd(&a.S[(size_t)(6*ib + r) * D + 6*ib + c], sB[w][lane]);
        if (ia >= 0 && ib >= 0) {
            if (ia > ib)      atomicAdd(&a.S[(size_t)(6*ia + r) * D + 6*ib + c], -sM[w][6*c + r]);   // B[a,b] = -M^T
            else if (ib > ia) atomicAdd(&a.S[(size_t)(6*ib + r) * D + 6*ia + c], -sM[w][6*r + c]);   // B[b,a] = -M
            else if (r >= c)  atomicAdd(&a.S[(size_t)(6*ia + r) * D + 6*ia + c], -(sM[w][6*r + c] + sM[w][6*c + r]));
        }
    } else if (lane < 42) {
        const int c = lane - 36;
        if (ia >= 0) {
            double v = 0.0;
            for (int s = 0; s < 6; ++s) v += sAd[w][6*s + c] * sg[w][s];
            atomicAdd(&a.y[6*ia + c], -v);
        }
        if (ib >= 0) atomicAdd(&a.y[6*ib + c], sg[w][c]);
    }
}

// ------------------------------------------------------------------ k_solve
// Damped, block-sparse (6x6 blocks) right-looking Cholesky of the reduced camera
// system, with y carried as an extra block row so the forward substitution is
// part of the factorisation.  A <- S + (ep + lm * diag S) I  (ba.py:67); a
// non-positive pivot gives dX = 0 (ba.py:9-13); a NaN in dX retries once with
// lm = 1e-3 (ba.py:324-325).  One workgroup; the factor lives in the workspace.
__device__ inline bool chol6_inv(float *Ablk, float *Linv) {
    // in: lower triangle of a 6x6 block (row-major).  out: L in place, L^-1 in Linv.
    float L[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) L[r][c] = c <= r ? Ablk[6*r + c] : 0.0f;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        float s = L[c][c];
#pragma unroll
        for (int k = 0; k < c; ++k) s -= L[c][k] * L[c][k];
        if (!(s > 0.0f)) ok = false;
        const float l = sqrtf(s), il = 1.0f / l;
        L[c][c] = l;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            float t = L[r][c];
#pragma unroll
            for (int k = 0; k < c; ++k) t -= L[r][k] * L[c][k];
            L[r][c] = t * il;
        }
    }
    float Li[6][6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (r < c) { Li[r][c] = 0.0f; continue; }
            float t = r == c ? 1.0f : 0.0f;
#pragma unroll
            for (int k = c; k < r; ++k) t -= L[r][k] * Li[k][c];
            Li[r][c] = t / L[r][r];
        }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) { Ablk[6*r + c] = L[r][c]; Linv[6*r + c] = Li[r][c]; }
    return ok;
}

// status word (int index) that k_refine_residual raises when the refinement has converged: the solve behind it returns at once
constexpr int kRefineDone = 210;

__global__ __launch_bounds__(1024) void k_solve_global(PlanDev pd, StepArgs a) {
    if (a.status[kRefineDone] != 0) return;
    __shared__ float part[kMaxFree * 6 + 6];
    __shared__ float tq[6];
    __shared__ int flags[2];          // [0] cholesky failed, [1] NaN in dX
    const int tid = threadIdx.x, nth = blockDim.x;
    const int n = pd.n, D = pd.D;
    float *Lw = a.lfac, *Li = a.linv, *z = a.zvec;
    int status = BT_SOLVE_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const float lm = attempt == 0 ? 1e-4f : 1e-3f;
        if (tid < 2) flags[tid] = 0;
        // load the structurally non-zero blocks of S (+ damping) and y
        for (int idx = tid; idx < pd.nnzb * 36; idx += nth) {
            const int b = idx / 36, e = idx % 36, r = e / 6, c = e % 6;
            const int row = pd.row_idx[b], col = pd.blk_col[b] & 255, src = pd.blk_src[b];
            const int rn = src >> 9, cn = (src >> 1) & 255;
            const int rr = (src & 1) ? c : r, cc = (src & 1) ? r : c;       // transposed source block
            double v = (row > col || r >= c) ? a.S[(size_t)(6*rn + rr) * D + 6*cn + cc] : 0.0;
            if (row == col && r == c) v = v + ((double)a.ep + (double)lm * v);
            Lw[idx] = (float)v;
        }
        for (int i = tid; i < D; i += nth) z[i] = (float)a.y[6 * pd.perm[i / 6] + i % 6];
        __syncthreads();

        for (int j = 0; j < n; ++j) {
            const int dpos = pd.col_ptr[j], cnt = pd.col_ptr[j + 1] - dpos - 1;
            if (tid == 0) {
                if (!chol6_inv(Lw + (size_t)dpos * 36, Li + (size_t)j * 36)) flags[0] = 1;
                float zz[6];
                for (int r = 0; r < 6; ++r) {                       // z_j <- L_jj^-1 z_j
                    float t = 0.0f;
                    for (int c = 0; c <= r; ++c) t += Li[j*36 + 6*r + c] * z[6*j + c];
                    zz[r] = t;
                }
                for (int r = 0; r < 6; ++r) z[6*j + r] = zz[r];
            }
            __syncthreads();
            // L_ij = A_ij L_jj^-T, one thread per block row; then y_i -= L_ij z_j
            for (int idx = tid; idx < cnt * 6; idx += nth) {
                const int s = idx / 6, r = idx % 6;
                float *blk = Lw + (size_t)(dpos + 1 + s) * 36 + 6*r;
                float in[6], out[6];
                for (int c = 0; c < 6; ++c) in[c] = blk[c];
                float dot = 0.0f;
                for (int c = 0; c < 6; ++c) {
                    float t = 0.0f;
                    for (int k = 0; k <= c; ++k) t += in[k] * Li[j*36 + 6*c + k];
                    out[c] = t;
                    dot += t * z[6*j + c];
                }
                for (int c = 0; c < 6; ++c) blk[c] = out[c];
                z[6 * pd.row_idx[dpos + 1 + s] + r] -= dot;
            }
            __syncthreads();
            const int u0 = pd.upd_ptr[j], nu = pd.upd_ptr[j + 1] - u0;
            for (int idx = tid; idx < nu * 36; idx += nth) {
                const int t = idx / 36, e = idx % 36, r = e / 6, c = e % 6;
                const int *tr = pd.upd + (size_t)(u0 + t) * 3;
                const float *L1 = Lw + (size_t)tr[0] * 36 + 6*r, *L2 = Lw + (size_t)tr[1] * 36 + 6*c;
                float acc = 0.0f;
                for (int k = 0; k < 6; ++k) acc += L1[k] * L2[k];
                Lw[(size_t)(tr[2] & 0x7fff) * 36 + e] -= acc;
            }
            __syncthreads();
        }

        // back substitution x = L^-T z, in place in z
        for (int j = n - 1; j >= 0; --j) {
            const int dpos = pd.col_ptr[j], cnt = pd.col_ptr[j + 1] - dpos - 1;
            for (int idx = tid; idx < cnt * 6; idx += nth) {
                const int s = idx / 6, c = idx % 6;
                const float *blk = Lw + (size_t)(dpos + 1 + s) * 36;
                const float *xr = z + 6 * pd.row_idx[dpos + 1 + s];
                float t = 0.0f;
                for (int r = 0; r < 6; ++r) t += blk[6*r + c] * xr[r];
                part[idx] = t;
            }
            __syncthreads();
            if (tid < 6) {
                float t = z[6*j + tid];
                for (int s = 0; s < cnt; ++s) t -= part[6*s + tid];
                tq[tid] = t;
            }
            __syncthreads();
            if (tid < 6) {
                float x = 0.0f;
                for (int r = tid; r < 6; ++r) x += Li[j*36 + 6*r + tid] * tq[r];
                z[6*j + tid] = x;
            }
            __syncthreads();
        }
        for (int i = tid; i < D; i += nth) if (z[i] != z[i]) flags[1] = 1;
        __syncthreads();
        const bool failed = flags[0] != 0, has_nan = flags[1] != 0;
        __syncthreads();
        if (failed) {                                   // zeros, and zeros hold no NaN: done
            for (int i = tid; i < D; i += nth) z[i] = 0.0f;
            status = BT_SOLVE_CHOL_FAILED;
            break;
        }
        if (!has_nan) break;
        status = BT_SOLVE_RETRIED;
    }
    __syncthreads();
    for (int i = tid; i < D; i += nth) a.dx[6 * pd.perm[i / 6] + i % 6] = z[i];
    if (tid == 0) a.status[0] = status;
}

// ------------------------------------------------------------------ k_solve_lds
// The same factorisation with the factor resident in LDS.  A lone wave retires
// roughly one instruction per 6-10 cycles on this part, so the sweep is written
// for the fewest instructions on the critical path, two short phases per column:
//   phase 1   wave 0: apply column j-1's update to the diagonal block of column j,
//             factor it (every lane redundantly, in registers), store L_jj;
//             all other waves: every other update of column j-1 (into column j's
//             sub-diagonal blocks, into later columns, and into y)
//   phase 2   all threads: one block row each of L_ij = A_ij L_jj^-T by forward
//             substitution; the extra row is y_j (forward substitution of the RHS)
// The diagonal block keeps L_jj with 1/l_cc on its diagonal.  After the sweep all
// threads bring the factor into back-substitution form (L_jj^-1 in the strict upper
// triangle of the diagonal block, M_ij = (L_ij L_jj^-1)^T), and wave 0 runs the
// sequential back substitution with DPP reductions.
#define BT_LT(r, c) ((r) * ((r) + 1) / 2 + (c))

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

// in place: lower triangle (packed) -> its Cholesky factor, diagonal entries hold 1 / l_cc.
template <typename T>
__device__ __forceinline__ bool chol6_packed(T (&L)[21]) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        T s = L[BT_LT(c, c)];
#pragma unroll
        for (int k = 0; k < c; ++k) s -= L[BT_LT(c, k)] * L[BT_LT(c, k)];
        ok = ok && (s > (T)0);
        const T il = rsqrt_t<T>(s);
        L[BT_LT(c, c)] = il;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            T t = L[BT_LT(r, c)];
#pragma unroll
            for (int k = 0; k < c; ++k) t -= L[BT_LT(r, k)] * L[BT_LT(c, k)];
            L[BT_LT(r, c)] = t * il;
        }
    }
    return ok;
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

size_t solve_lds_bytes(const PlanDev &pd, size_t elem) {
    return solve_lds_bytes_raw((size_t)pd.nnzb, (size_t)pd.D, (size_t)pd.nupd, (size_t)pd.n, (size_t)pd.nlev, (size_t)pd.ndp, elem);
}

template <typename T> __device__ __forceinline__ void lds_sub(T *p, T v, bool atomic) {
    if (atomic) atomicAdd(p, -v); else *p -= v;
}

// One ROW of an update triple: dst[r][:] -= (row r of block tr[0]) . (rows of block tr[1])^T.
// 21 vector LDS loads and 36 FMAs for 6 outputs.  Bit 15 of tr[2]: the destination is also
// updated by another column of the same level -> LDS atomics.
// (the triple as three values: callers that keep it packed in one 8-byte LDS word)
template <typename T>
__device__ __forceinline__ void apply_update_row3(T *Lw, unsigned s1, unsigned s2, unsigned d, int r) {
    T a[6], b[36], o[6], v[6];
    T *dst = Lw + (d & 0x7fffu) * 36 + 6 * r;
    const T *bb = Lw + s2 * 36;
    load_row6(Lw + s1 * 36 + 6 * r, a);
#pragma unroll
    for (int c = 0; c < 6; ++c) load_row6(bb + 6 * c, reinterpret_cast<T (&)[6]>(b[6 * c]));
    load_row6(dst, v);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        T acc = a[0] * b[6 * c];
#pragma unroll
        for (int k = 1; k < 6; ++k) acc += a[k] * b[6 * c + k];
        o[c] = acc;
    }
    if (d & 0x8000u) {
#pragma unroll
        for (int c = 0; c < 6; ++c) atomicAdd(dst + c, -o[c]);
    } else {
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] -= o[c];
        store_row6(dst, v);
    }
}

template <typename T, bool PROF = false>
__device__ __forceinline__ void apply_update_row(T *Lw, const unsigned short *tr, int r, long long *pf = nullptr, long long *tcp = nullptr) {
    T a[6], b[36], o[6], v[6];
    const unsigned d = tr[2];
    if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long tn = clock64(); pf[2] += tn - *tcp; *tcp = tn; }
    T *dst = Lw + (size_t)(d & 0x7fffu) * 36 + 6 * r;
    const T *bb = Lw + (size_t)tr[1] * 36;
    // all 24 vector loads are issued before any arithmetic: one LDS latency instead of one per row
    load_row6(Lw + (size_t)tr[0] * 36 + 6 * r, a);
#pragma unroll
    for (int c = 0; c < 6; ++c) load_row6(bb + 6 * c, reinterpret_cast<T (&)[6]>(b[6 * c]));
    load_row6(dst, v);
    __builtin_amdgcn_sched_barrier(0);
    if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long tn = clock64(); pf[4] += tn - *tcp; *tcp = tn; }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        T acc = a[0] * b[6 * c];
#pragma unroll
        for (int k = 1; k < 6; ++k) acc += a[k] * b[6 * c + k];
        o[c] = acc;
    }
    if (d & 0x8000u) {
#pragma unroll
        for (int c = 0; c < 6; ++c) atomicAdd(dst + c, -o[c]);
    } else {
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] -= o[c];
        store_row6(dst, v);
    }
    if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long tn = clock64(); pf[9] += tn - *tcp; *tcp = tn; }
}

// wave-uniform metadata: LDS -> SGPRs
__device__ __forceinline__ int4 uniform4(const int4 v) {
    return make_int4(__builtin_amdgcn_readfirstlane(v.x), __builtin_amdgcn_readfirstlane(v.y),
                     __builtin_amdgcn_readfirstlane(v.z), __builtin_amdgcn_readfirstlane(v.w));
}

template <typename T, bool PROF>
__global__ __launch_bounds__(768) void k_solve_lds(PlanDev pd, StepArgs a) {
    if (sizeof(T) == 4 && a.status[kRefineDone] != 0) return;       // (the double factor solves once: no refinement, no flag)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int flags[2];
    const int tid = threadIdx.x, nth = blockDim.x, wave = tid >> 6, lane = tid & 63;
    const int n = pd.n, D = pd.D, nnzb = pd.nnzb, nlev = pd.nlev;
    T *Lw = reinterpret_cast<T *>(smem);
    T *z = Lw + (size_t)nnzb * 36, *zt = z + D;
    size_t off = (((size_t)nnzb * 36 + 2 * (size_t)D) * sizeof(T) + 15) / 16 * 16;
    unsigned short *upd = reinterpret_cast<unsigned short *>(smem + off);
    off = (off + (size_t)pd.nupd * 3 * sizeof(unsigned short) + 15) / 16 * 16;
    int *row_idx = reinterpret_cast<int *>(smem + off), *col_ptr = row_idx + nnzb, *upd_ptr = col_ptr + n + 1,
        *upd_next = upd_ptr + n + 1, *dp_ptr = upd_next + n + 1, *lvl_ptr = dp_ptr + n + 1,
        *lvl_cols = lvl_ptr + nlev + 1, *dp = lvl_cols + n;
    int4 *lvl_meta = reinterpret_cast<int4 *>(smem + ((reinterpret_cast<unsigned char *>(dp + pd.ndp) - smem + 15) / 16 * 16));
    long long pf[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tc = PROF ? clock64() : 0, tn;
#define BT_PF(i) do { if (PROF) { tn = clock64(); pf[i] += tn - tc; tc = tn; } } while (0)
    for (int i = tid; i < pd.nupd * 3; i += nth) upd[i] = (unsigned short)pd.upd[i];
    for (int i = tid; i < nnzb; i += nth) row_idx[i] = pd.row_idx[i] | (pd.blk_col[i] << 8);   // row | col << 8 | shared-y << 24
    for (int i = tid; i <= n; i += nth) {
        col_ptr[i] = pd.col_ptr[i]; upd_ptr[i] = pd.upd_ptr[i]; upd_next[i] = pd.upd_next[i]; dp_ptr[i] = pd.dp_ptr[i];
    }
    for (int i = tid; i <= nlev; i += nth) lvl_ptr[i] = pd.lvl_ptr[i];
    for (int i = tid; i < n; i += nth) lvl_cols[i] = pd.lvl_cols[i];
    for (int i = tid; i < pd.ndp; i += nth) dp[i] = pd.dp[i];
    for (int i = tid; i < nlev * kMaxLevelCols * 2; i += nth) lvl_meta[i] = reinterpret_cast<const int4 *>(pd.lvl_meta)[i];
    __syncthreads();

    int status = BT_SOLVE_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const double lm = attempt == 0 ? 1e-4 : 1e-3;
        if (tid < 2) flags[tid] = 0;
        // one thread per block row: 6 doubles of S (caller order, lower triangle; blk_src says where
        // and whether transposed); 4 rounds of loads in flight
        for (int base = 0; base < nnzb * 6; base += 2 * nth) {
            double v[2][6];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int idx = base + u * nth + tid;
                if (idx < nnzb * 6) {
                    const int b = idx / 6, r = idx - 6 * b, src = pd.blk_src[b];
                    const int rn = src >> 9, cn = (src >> 1) & 255;
                    if (src & 1) {
#pragma unroll
                        for (int c = 0; c < 6; ++c) v[u][c] = a.S[(size_t)(6 * rn + c) * D + 6 * cn + r];
                    } else {
                        const double *p = a.S + (size_t)(6 * rn + r) * D + 6 * cn;
#pragma unroll
                        for (int c = 0; c < 6; ++c) v[u][c] = p[c];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int idx = base + u * nth + tid;
                if (idx < nnzb * 6) {
                    const int b = idx / 6, r = idx - 6 * b, rc = row_idx[b];
                    const bool diag = (rc & 255) == ((rc >> 8) & 255);
                    T w[6];
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
                        double x = (!diag || r >= c) ? v[u][c] : 0.0;
                        if (diag && r == c) x = x + ((double)a.ep + lm * x);          // ba.py:67
                        w[c] = (T)x;
                    }
                    store_row6(Lw + (size_t)b * 36 + 6 * r, w);
                }
            }
        }
        for (int i = tid; i < D; i += nth) z[i] = (T)a.y[6 * pd.perm[i / 6] + i % 6];
        __syncthreads();
        BT_PF(0);

        // Per-level metadata (wave-uniform, kept in SGPRs).  The entry of level l+1 is fetched from LDS
        // before the barrier that ends level l, so its latency hides behind the barrier.
        int4 cA0, cA1, cA2, cA3, pA0, pA1, pA2, pA3, cW, cWb;     // current / previous level, and this wave's own column
        int cn0, cn1, cn2, cn3, pn0 = 0, pn1 = 0, pn2 = 0, pn3 = 0, nc;
        pA0 = pA1 = pA2 = pA3 = make_int4(-1, 0, 0, 0);
        auto fetch_level = [&](int l) {
            const int4 *ml = lvl_meta + (size_t)l * kMaxLevelCols * 2;
            cA0 = uniform4(ml[0]); cA1 = uniform4(ml[2]); cA2 = uniform4(ml[4]); cA3 = uniform4(ml[6]);
            const int4 b0 = uniform4(ml[1]);
            cn0 = b0.x; nc = b0.w;
            cn1 = __builtin_amdgcn_readfirstlane(ml[3].x); cn2 = __builtin_amdgcn_readfirstlane(ml[5].x);
            cn3 = __builtin_amdgcn_readfirstlane(ml[7].x);
            const int wq = wave < kMaxLevelCols ? wave : 0;
            cW = uniform4(ml[2 * wq]); cWb = uniform4(ml[2 * wq + 1]);
        };
        fetch_level(0);
        long long ph1 = 0, ph2 = 0, tph = PROF ? clock64() : 0;
        for (int l = 0; l < nlev; ++l) {
            if (PROF) tph = clock64();
            // ---- phase 1
            if (wave < nc) {
                __builtin_amdgcn_s_setprio(3);            // the critical path of the level: win issue arbitration on this SIMD
                const int4 ma = cW, mb = cWb;
                const int dpos = ma.y;
                for (int k = mb.y; k < mb.y + mb.z; ++k) {        // pending updates of this column's diagonal block
                    if (lane < 36) {
                        const unsigned short *tr = upd + 3 * dp[k];
                        const int r = lane / 6, c = lane - 6 * r;
                        const T *src = Lw + (size_t)tr[0] * 36;
                        T x[6], y[6];
                        load_row6(src + 6 * r, x);
                        load_row6(src + 6 * c, y);
                        T acc = x[0] * y[0];
#pragma unroll
                        for (int q = 1; q < 6; ++q) acc += x[q] * y[q];
                        Lw[(size_t)dpos * 36 + lane] -= acc;
                    }
                    wave_fence();
                }
                T L[21];
                const T *dblk = Lw + (size_t)dpos * 36;
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    T row[6];
                    load_row6(dblk + 6 * r, row);
#pragma unroll
                    for (int c = 0; c <= r; ++c) L[BT_LT(r, c)] = row[c];
                }
                const bool ok = chol6_packed<T>(L);
                BT_PF(2);
                if (lane == 0) {                 // entries above the diagonal are don't-care until Linv is put there
                    if (!ok) flags[0] = 1;
#pragma unroll
                    for (int r = 0; r < 6; ++r) {
                        T row[6];
#pragma unroll
                        for (int c = 0; c < 6; ++c) row[c] = L[BT_LT(r, c <= r ? c : r)];
                        store_row6(Lw + (size_t)dpos * 36 + 6 * r, row);
                    }
                }
                BT_PF(4);
                __builtin_amdgcn_s_setprio(0);
            } else if (l > 0) {
                // the other update triples of the previous level's columns (one ROW of a triple per
                // thread) and their contribution to y, all columns flattened over the helper threads
                const int h = tid - 64 * nc, hs = nth - 64 * nc;
                const int nu0 = pn0, nu1 = pn1, nu2 = pn2, nu3 = pn3;
                // (a) update rows of all columns of the previous level, flattened over the helper threads
                int rows_b[kMaxLevelCols + 1];
                rows_b[0] = 0;
                rows_b[1] = pA0.x >= 0 ? nu0 * 6 : 0;
                rows_b[2] = rows_b[1] + (pA1.x >= 0 ? nu1 * 6 : 0);
                rows_b[3] = rows_b[2] + (pA2.x >= 0 ? nu2 * 6 : 0);
                rows_b[4] = rows_b[3] + (pA3.x >= 0 ? nu3 * 6 : 0);
                BT_PF(0);                 // (helper waves: slot 0 = time from the barrier to the first item)
                for (int item = h; item < rows_b[kMaxLevelCols]; item += hs) {
                    int q = 0;
#pragma unroll
                    for (int k = 1; k < kMaxLevelCols; ++k) q += item >= rows_b[k] ? 1 : 0;
                    const int idx = item - (q == 0 ? 0 : q == 1 ? rows_b[1] : q == 2 ? rows_b[2] : rows_b[3]);
                    const int4 pa = q == 0 ? pA0 : q == 1 ? pA1 : q == 2 ? pA2 : pA3;
                    const int t = idx / 6;
                    apply_update_row<T, PROF>(Lw, upd + 3 * (pa.w + t), idx - 6 * t, pf, &tc);
                }
                // (b) their contribution to y, on the waves after those that had update rows (no wave
                //     runs both kinds of item in the common one-round case)
                int ys_b[kMaxLevelCols + 1];
                ys_b[0] = 0;
                ys_b[1] = pA0.x >= 0 ? pA0.z * 6 : 0;
                ys_b[2] = ys_b[1] + (pA1.x >= 0 ? pA1.z * 6 : 0);
                ys_b[3] = ys_b[2] + (pA2.x >= 0 ? pA2.z * 6 : 0);
                ys_b[4] = ys_b[3] + (pA3.x >= 0 ? pA3.z * 6 : 0);
                const int shift = ((rows_b[kMaxLevelCols] + 63) >> 6) << 6;
                for (int item = (h - shift % hs + hs) % hs; item < ys_b[kMaxLevelCols]; item += hs) {
                    int q = 0;
#pragma unroll
                    for (int k = 1; k < kMaxLevelCols; ++k) q += item >= ys_b[k] ? 1 : 0;
                    const int qq = item - (q == 0 ? 0 : q == 1 ? ys_b[1] : q == 2 ? ys_b[2] : ys_b[3]);
                    const int4 pa = q == 0 ? pA0 : q == 1 ? pA1 : q == 2 ? pA2 : pA3;
                    const int pj = pa.x, dposp = pa.y, sb = qq / 6, r = qq - 6 * sb;
                    T lr[6], zr[6];
                    load_row6(Lw + (size_t)(dposp + 1 + sb) * 36 + 6 * r, lr);
                    load_row6(z + 6 * pj, zr);
                    T acc = lr[0] * zr[0];
#pragma unroll
                    for (int k = 1; k < 6; ++k) acc += lr[k] * zr[k];
                    const int rcv = row_idx[dposp + 1 + sb];
                    lds_sub(z + 6 * (rcv & 255) + r, acc, (rcv >> 24) != 0);
                }
                BT_PF(1);
            }
            if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); ph1 += clock64() - tph; }
            __syncthreads();
            if (PROF) tph = clock64();
            BT_PF(5);
            // ---- phase 2: block rows of the level's columns (and their y) by forward substitution
            {
                const int4 mA0 = cA0, mA1 = cA1, mA2 = cA2, mA3 = cA3;
                int rows_before[kMaxLevelCols + 1];
                rows_before[0] = 0;
                rows_before[1] = mA0.x >= 0 ? mA0.z * 6 + 1 : 0;
                rows_before[2] = rows_before[1] + (mA1.x >= 0 ? mA1.z * 6 + 1 : 0);
                rows_before[3] = rows_before[2] + (mA2.x >= 0 ? mA2.z * 6 + 1 : 0);
                rows_before[4] = rows_before[3] + (mA3.x >= 0 ? mA3.z * 6 + 1 : 0);
                for (int item = tid; item < rows_before[kMaxLevelCols]; item += nth) {
                    int q = 0;
#pragma unroll
                    for (int k = 1; k < kMaxLevelCols; ++k) q += item >= rows_before[k] ? 1 : 0;
                    const int rw = item - (q == 0 ? 0 : q == 1 ? rows_before[1] : q == 2 ? rows_before[2] : rows_before[3]);
                    const int4 ma = q == 0 ? mA0 : q == 1 ? mA1 : q == 2 ? mA2 : mA3;
                    const int j = ma.x, dpos = ma.y, cnt = ma.z;
                    T L[21];
                    const T *dblk = Lw + (size_t)dpos * 36;
#pragma unroll
                    for (int r = 0; r < 6; ++r) {
                        T row[6];
                        load_row6(dblk + 6 * r, row);
#pragma unroll
                        for (int c = 0; c <= r; ++c) L[BT_LT(r, c)] = row[c];
                    }
                    T *p = rw < cnt * 6 ? Lw + (size_t)(dpos + 1) * 36 + 6 * rw : z + 6 * j;
                    T in[6], out[6];
                    load_row6(p, in);
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
                        T t = in[c];
#pragma unroll
                        for (int k = 0; k < c; ++k) t -= out[k] * L[BT_LT(c, k)];
                        out[c] = t * L[BT_LT(c, c)];
                    }
                    store_row6(p, out);
                }
            }
            BT_PF(3);
            if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); ph2 += clock64() - tph; }
            pA0 = cA0; pA1 = cA1; pA2 = cA2; pA3 = cA3; pn0 = cn0; pn1 = cn1; pn2 = cn2; pn3 = cn3;
            if (l + 1 < nlev) fetch_level(l + 1);
            __syncthreads();
            BT_PF(5);
        }

        if (PROF && lane == 0) {
            long long *o = reinterpret_cast<long long *>(a.status + 4) + 40 + wave * 2;
            o[0] = ph1; o[1] = ph2;
        }
        // ---- back-substitution form
        // (a) L_jj^-1 into the strict upper triangle of the diagonal block (one thread per column)
        for (int j = tid; j < n; j += nth) {
            T *dblk = Lw + (size_t)col_ptr[j] * 36;
            T L[21], li[21];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) L[BT_LT(r, c)] = dblk[6 * r + c];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                li[BT_LT(c, c)] = L[BT_LT(c, c)];
#pragma unroll
                for (int r = c + 1; r < 6; ++r) {
                    T t = (T)0;
#pragma unroll
                    for (int k = c; k < r; ++k) t += L[BT_LT(r, k)] * li[BT_LT(k, c)];
                    li[BT_LT(r, c)] = -t * L[BT_LT(r, r)];
                }
            }
#pragma unroll
            for (int r = 1; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < r; ++c) dblk[6 * c + r] = li[BT_LT(r, c)];      // Linv[r][c] at [c][r]
        }
        __syncthreads();
        // (b) block rows: Mt[r][c] = sum_{k>=c} Linv_j[k][c] L_ij[r][k];  zt_j[c] = sum_{k>=c} Linv_j[k][c] z_j[k]
        for (int idx = tid; idx < nnzb * 6 + n; idx += nth) {
            int j;
            T *p, *q;
            if (idx < nnzb * 6) {
                const int b = idx / 6, r = idx - 6 * b;
                j = (row_idx[b] >> 8) & 255;
                if ((row_idx[b] & 255) == j) continue;
                p = Lw + (size_t)b * 36 + 6 * r; q = p;
            } else {
                j = idx - nnzb * 6;
                p = z + 6 * j; q = zt + 6 * j;
            }
            const T *dblk = Lw + (size_t)col_ptr[j] * 36;
            T in[6], out[6];
            load_row6(p, in);
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                T t = dblk[7 * c] * in[c];
#pragma unroll
                for (int k = c + 1; k < 6; ++k) t += dblk[6 * c + k] * in[k];
                out[c] = t;
            }
            store_row6(q, out);
        }
        __syncthreads();
        BT_PF(6);
        // (c) x_j = zt_j - sum_{i>j} M_ij x_i, levels descending; one wave per column of the level,
        //     lane = (component c) * 8 + g
        for (int l = nlev - 1; l >= 0; --l) {
            const int4 ma = uniform4(lvl_meta[(l * kMaxLevelCols + (wave < kMaxLevelCols ? wave : 0)) * 2]);
            if (wave < kMaxLevelCols && ma.x >= 0) {
                const int c = lane >> 3, g = lane & 7;
                const int j = ma.x, dpos = ma.y, cnt = ma.z;
                T acc = (T)0;
                if (c < 6)
                    for (int sb = g; sb < cnt; sb += 8) {           // one sub-block per lane group
                        const int b = dpos + 1 + sb;
                        T x[6];
                        load_row6(zt + 6 * (row_idx[b] & 255), x);
                        const T *mb = Lw + (size_t)b * 36 + c;     // Mt[r][c]
                        acc += mb[0] * x[0] + mb[6] * x[1] + mb[12] * x[2] + mb[18] * x[3] + mb[24] * x[4] + mb[30] * x[5];
                    }
                acc = dpp_add8(acc);
                if (c < 6 && g == 0) zt[6 * j + c] -= acc;
            }
            __syncthreads();
        }
        BT_PF(7);
        for (int i = tid; i < D; i += nth) if (zt[i] != zt[i]) flags[1] = 1;
        __syncthreads();
        const bool failed = flags[0] != 0, has_nan = flags[1] != 0;
        __syncthreads();
        if (failed) {
            for (int i = tid; i < D; i += nth) zt[i] = (T)0;
            status = BT_SOLVE_CHOL_FAILED;
            break;
        }
        if (!has_nan) break;
        status = BT_SOLVE_RETRIED;
    }
    __syncthreads();
    for (int i = tid; i < D; i += nth) a.dx[6 * pd.perm[i / 6] + i % 6] = (float)zt[i];
    if (tid == 0) a.status[0] = status;
    BT_PF(8);
    if (PROF && lane == 0 && (wave == 0 || wave == 2)) {        // measurement only: phase cycle counts of a critical and a helper wave
        long long *o = reinterpret_cast<long long *>(a.status + 4) + (wave ? 1 : 0) * 10;
        for (int i = 0; i < 10; ++i) o[i] = pf[i];
    }
#undef BT_PF
}

// ------------------------------------------------------------------ k_solve_fused
// The LDS-resident factorisation with ONE phase and one barrier per level (levels of at most
// two columns: two-ended chains).  Updates are split by destination (ba_plan.cpp, fz_*):
// "pending" = the destination column is factored in the very next level, "lazy" = later.
//   diagonal wave  one per column: lanes 0..35 apply the pending updates to the column's diagonal
//                  block (one element each) and publish it through LDS + a flag
//   row waves      64 panel rows of one column each (metadata stays scalar): every lane applies
//                  the pending update of its own row (or of y_j) in registers - all loads in
//                  flight before the first FMA - while the diagonal wave works, then picks up the
//                  block, factors it redundantly in registers and forward-substitutes its row
//   helper waves   the lazy updates of the level below (one row of a triple per thread) and its
//                  lazy y contributions
// Against k_solve_lds (two phases: factor | substitute) this removes a barrier, the store and
// reload of L_jj between the phases and the wait of the substitution for the slowest helper.
// The sweep is bounded by LDS throughput (~175 KB of 16-byte reads per level, with bank conflicts
// between the 288-byte blocks) about as much as by the 6x6 chain; see DESIGN.md section 6.
constexpr int kLoadInFlight = 4;      // block rows of S a thread has in flight (6 doubles each)

template <typename T>
__device__ __forceinline__ void lds_load_system(const PlanDev &pd, const StepArgs &a, T *Lw, T *z, double lm, int tid, int nth) {
    // reads global memory only (the block's place in S says whether it is a diagonal block), so the loads are in
    // flight together with the table copies that precede the call; the caller's barrier covers both
    const int nnzb = pd.nnzb, D = pd.D;
    for (int base = 0; base < nnzb * 6; base += kLoadInFlight * nth) {
        double v[kLoadInFlight][6];
        bool dg[kLoadInFlight];
#pragma unroll
        for (int u = 0; u < kLoadInFlight; ++u) {
            const int idx = base + u * nth + tid;
            if (idx < nnzb * 6) {
                const int b = idx / 6, r = idx - 6 * b, src = pd.blk_src[b];
                const int rn = src >> 9, cn = (src >> 1) & 255;
                dg[u] = rn == cn;
                if (src & 1) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) v[u][c] = a.S[(size_t)(6 * rn + c) * D + 6 * cn + r];
                } else {
                    const double *p = a.S + (size_t)(6 * rn + r) * D + 6 * cn;
#pragma unroll
                    for (int c = 0; c < 6; ++c) v[u][c] = p[c];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kLoadInFlight; ++u) {
            const int idx = base + u * nth + tid;
            if (idx < nnzb * 6) {
                const int b = idx / 6, r = idx - 6 * b;
                const bool diag = dg[u];
                T w[6];
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    double x = (!diag || r >= c) ? v[u][c] : 0.0;
                    if (diag && r == c) x = x + ((double)a.ep + lm * x);          // ba.py:67
                    w[c] = (T)x;
                }
                store_row6(Lw + (size_t)b * 36 + 6 * r, w);
            }
        }
    }
    for (int i = tid; i < D; i += nth) z[i] = (T)a.y[6 * pd.perm[i / 6] + i % 6];
}

// [S | y] -> LDS in factor order by LDS-DMA (global_load_lds_dwordx4: no staging registers, every piece of the system in
// flight at once).  A 16-byte piece = third h of row r of block b, piece index 18 b + 3 r + h — which IS its place in the
// factor's LDS image (block b at 288 b bytes, rows of 48 bytes), so a wave instruction deposits 64 consecutive pieces at a
// wave-uniform base + lane * 16 as the instruction requires, each lane fetching from its own place in S.  Blocks that S
// holds transposed (its lower triangle, in the caller's pose order) and the diagonal blocks (upper triangle cleared,
// damping ba.py:67) are put right afterwards in LDS (sys_dma_fixup).  `bsrc`: the plan's blk_src, copied to LDS beforehand.
template <typename T>
__device__ __forceinline__ void sys_dma_issue(const PlanDev &pd, const StepArgs &a, T *Lw, const int *bsrc, int wave, int lane, int nw) {
    static_assert(sizeof(T) == 8, "double factor");
    const int total = pd.nnzb * 18;
    const unsigned D = (unsigned)pd.D;
    for (int k = wave; k * 64 < total; k += nw) {
        const int idx = k * 64 + lane;
        if (idx < total) {
            const int b = idx / 18, rem = idx - 18 * b, r = rem / 3, h = rem - 3 * r;
            const unsigned src = (unsigned)bsrc[b], rn = src >> 9, cn = (src >> 1) & 255u;
            const double *g = a.S + ((6u * rn + (unsigned)r) * D + 6u * cn + 2u * (unsigned)h);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                             (__attribute__((address_space(3))) void *)(Lw + (size_t)k * 128), 16, 0, 0);
        }
    }
}
// After the DMA: the blocks S holds transposed, one thread per (block of the list `trl`, row r < 5) — its up to five
// (r, c > r) / (c, r) swaps with all reads in flight before the writes —, and the damping of the diagonal (ba.py:67), one
// thread per diagonal element.  The upper triangles of the diagonal blocks stay as they came (S keeps its lower triangle
// only): nothing reads them — the column wave's lanes carry them along as dead values, the back substitution overwrites
// them with L^-1.
template <typename T>
__device__ __forceinline__ void sys_dma_fixup(const PlanDev &pd, const StepArgs &a, T *Lw, const int *trl, int ntr, const int *col_ptr, double lm, bool zero_upper, int tid, int nth) {
    for (int it = tid; it < ntr * 5; it += nth) {
        const int li = it / 5, r = it - 5 * li;
        T *blk = Lw + trl[li] * 36;
        T lo[5], up[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) if (r + 1 + k < 6) { lo[k] = blk[6 * (r + 1 + k) + r]; up[k] = blk[6 * r + r + 1 + k]; }
#pragma unroll
        for (int k = 0; k < 5; ++k) if (r + 1 + k < 6) { blk[6 * (r + 1 + k) + r] = up[k]; blk[6 * r + r + 1 + k] = lo[k]; }
    }
    for (int it = tid; it < pd.D; it += nth) {
        T *dptr = Lw + col_ptr[it / 6] * 36 + 7 * (it % 6);
        const T x = *dptr;
        *dptr = x + ((T)a.ep + (T)lm * x);
    }
    if (zero_upper)
        for (int it = tid; it < pd.n * 15; it += nth) {
            const int jb = it / 15, e = it - 15 * jb, r = e >= 10 ? 5 : e >= 6 ? 4 : e >= 3 ? 3 : e >= 1 ? 2 : 1, c = e - r * (r - 1) / 2;
            Lw[col_ptr[jb] * 36 + 6 * c + r] = (T)0;
        }
}

// The whole load for the LDS-resident double-precision solvers: global memory in two round trips (the plan's tables — static,
// L2-resident — among them blk_src; then [S | y], which other chips' atomics have just accumulated and which comes from the
// memory side) instead of lds_load_system's chain of dependent ones (13.6k -> 9k cycles at 64 keyframes incl. the fix-up).
// Contains workgroup barriers; the caller's barrier after it covers the fix-up.  `col_ptr`: the LDS copy.
template <typename T>
__device__ __forceinline__ void lds_load_system_dma(const PlanDev &pd, const StepArgs &a, T *Lw, T *z, int *bsrc, int *trl, int *ntr, const int *col_ptr,
                                                    double lm, bool first, bool zero_upper, int tid, int nth) {
    const int wave = tid >> 6, lane = tid & 63, nw = nth >> 6, D = pd.D;
    const int yperm = tid < D ? pd.perm[tid / 6] : 0;
    if (first) {
        if (tid == 0) *ntr = 0;
        __syncthreads();
        for (int i = tid; i < pd.nnzb; i += nth) {
            const int src = pd.blk_src[i];
            bsrc[i] = src;
            if (src & 1) trl[atomicAdd(ntr, 1)] = i;          // the blocks S holds transposed (any order)
        }
    }
    __syncthreads();
    sys_dma_issue<T>(pd, a, Lw, bsrc, wave, lane, nw);
    if (tid < D) z[tid] = (T)a.y[6 * yperm + tid % 6];
    for (int i = tid + nth; i < D; i += nth) z[i] = (T)a.y[6 * pd.perm[i / 6] + i % 6];
    __syncthreads();                                      // (waits for the wave's DMA as well: vmcnt(0) in front of the barrier)
    sys_dma_fixup<T>(pd, a, Lw, trl, *ntr, col_ptr, lm, zero_upper, tid, nth);
}


// Back substitution of the LDS-resident factor (diagonal blocks hold L_jj with 1/l_cc on the
// diagonal): brings it into M form, then x_j = zt_j - sum_{i>j} M_ij x_i by levels, descending.
template <typename T, bool RAW_DIAG = false>
__device__ __forceinline__ void lds_back_substitute(const PlanDev &pd, T *Lw, T *z, T *zt, const int *row_idx,
                                                    const int *col_ptr, const int4 *lvl_meta, int mstride, int tid, int nth, long long *tprof = nullptr) {
    const int n = pd.n, nnzb = pd.nnzb, nlev = pd.nlev, wave = tid >> 6, lane = tid & 63;
    for (int j = tid; j < n; j += nth) {
        T *dblk = Lw + (size_t)col_ptr[j] * 36;
        T L[21], li[21];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) L[BT_LT(r, c)] = dblk[6 * r + c];
        if (RAW_DIAG) {                   // the block still holds the (fully updated) A_jj: factor it here
            (void)chol6_packed<T>(L);
#pragma unroll
            for (int c = 0; c < 6; ++c) dblk[7 * c] = L[BT_LT(c, c)];
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            li[BT_LT(c, c)] = L[BT_LT(c, c)];
#pragma unroll
            for (int r = c + 1; r < 6; ++r) {
                T t = (T)0;
#pragma unroll
                for (int k = c; k < r; ++k) t += L[BT_LT(r, k)] * li[BT_LT(k, c)];
                li[BT_LT(r, c)] = -t * L[BT_LT(r, r)];
            }
        }
#pragma unroll
        for (int r = 1; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < r; ++c) dblk[6 * c + r] = li[BT_LT(r, c)];      // Linv[r][c] at [c][r]
    }
    __syncthreads();
    if (tprof) tprof[0] = clock64();
    for (int idx = tid; idx < nnzb * 6 + n; idx += nth) {
        int j;
        T *p, *q;
        if (idx < nnzb * 6) {
            const int b = idx / 6, r = idx - 6 * b;
            j = (row_idx[b] >> 8) & 255;
            if ((row_idx[b] & 255) == j) continue;
            p = Lw + (size_t)b * 36 + 6 * r; q = p;
        } else {
            j = idx - nnzb * 6;
            p = z + 6 * j; q = zt + 6 * j;
        }
        const T *dblk = Lw + (size_t)col_ptr[j] * 36;
        T in[6], out[6];
        load_row6(p, in);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            T t = dblk[7 * c] * in[c];
#pragma unroll
            for (int k = c + 1; k < 6; ++k) t += dblk[6 * c + k] * in[k];
            out[c] = t;
        }
        store_row6(q, out);
    }
    __syncthreads();
    if (tprof) tprof[1] = clock64();
    // (c) x_j = zt_j - sum_{i>j} M_ij x_i, levels descending, ONE WAVE PER COLUMN SLOT and no barrier unless
    // the level reads an x_i another slot's wave wrote since the last barrier (lvl_meta[..].w, ba_plan.cpp
    // bs_sync): on a two-ended chain the two waves run down their chains independently.  The static
    // operands of level l - 1 (block index, M entries) are loaded before level l's x are waited for.
    // lane = (component c) * 8 + g, one sub-block per lane group g.
    {
        const bool bw = wave < kMaxLevelCols;
        const int c = lane >> 3, g = lane & 7;
        struct Pre { int4 ma; int rc; T m[6]; T ztj; };
        auto preload = [&](int l, Pre &P) {           // everything of level l that does not depend on the x computed so far
            // (per-lane copies of the level record: no scalarisation needed; operands of lanes without a
            //  sub-block are never used)
            P.ma = lvl_meta[(l * kMaxLevelCols + (bw ? wave : 0)) * mstride];
            if (!bw) P.ma.x = -1;
            if (P.ma.x >= 0 && c < 6) {
                P.ztj = zt[6 * P.ma.x + c];
                if (g < P.ma.z) {
                    const int b = P.ma.y + 1 + g;
                    P.rc = row_idx[b] & 255;
                    const T *mb = Lw + (size_t)b * 36 + c;     // Mt[r][c]
#pragma unroll
                    for (int k = 0; k < 6; ++k) P.m[k] = mb[6 * k];
                }
            }
        };
        auto step = [&](const Pre &P) {
            if (__builtin_amdgcn_readfirstlane(P.ma.w)) __syncthreads();
            if (P.ma.x >= 0) {
                const int j = P.ma.x, dpos = P.ma.y, cnt = P.ma.z;
                T acc = (T)0;
                if (c < 6 && g < cnt) {
                    T x[6];
                    load_row6(zt + 6 * P.rc, x);
                    acc = P.m[0] * x[0] + P.m[1] * x[1] + P.m[2] * x[2] + P.m[3] * x[3] + P.m[4] * x[4] + P.m[5] * x[5];
                    for (int sb = g + 8; sb < cnt; sb += 8) {       // wide columns: further sub-blocks of this lane group
                        const int b = dpos + 1 + sb;
                        load_row6(zt + 6 * (row_idx[b] & 255), x);
                        const T *mb = Lw + (size_t)b * 36 + c;
                        acc += mb[0] * x[0] + mb[6] * x[1] + mb[12] * x[2] + mb[18] * x[3] + mb[24] * x[4] + mb[30] * x[5];
                    }
                }
                acc = dpp_add8(acc);
                if (c < 6 && g == 0) zt[6 * j + c] = P.ztj - acc;
                wave_fence();
            }
        };
        Pre A = {}, B = {};                            // two register sets, levels alternate between them
        preload(nlev - 1, A);
        for (int l = nlev - 1; l >= 0; l -= 2) {
            if (l >= 1) preload(l - 1, B);
            step(A);
            if (l >= 1) {
                if (l >= 2) preload(l - 2, A);
                step(B);
            }
        }
        __syncthreads();
    }
}

// LDS of k_solve_fused: Lw | z | work | row_idx | pfirst | col_ptr, where `work` holds the sweep's tables
// (published diagonal blocks, lazy triples) and is reused for zt afterwards.
// The per-level metadata stays in global memory (prefetched a level ahead).
__host__ __device__ inline size_t fused_work_bytes(const PlanDev &pd, int nthreads) {
    (void)nthreads;
    const size_t b = 2 * 36 * sizeof(double) +          // published diagonal blocks of the level's two columns

                     (size_t)pd.fz_nlazy * 4 * sizeof(unsigned short) + 16;
    const size_t zt = (size_t)pd.D * sizeof(double) + (size_t)pd.nlev * kMaxLevelCols * sizeof(int4);   // zt + compact level table
    return ((b > zt ? b : zt) + 15) / 16 * 16;
}
size_t solve_fused_lds_bytes(const PlanDev &pd, int nthreads) {
    return ((size_t)pd.nnzb * 36 + (size_t)pd.D) * sizeof(double) + fused_work_bytes(pd, nthreads) +
           (5 * (size_t)pd.nnzb + (size_t)pd.n + 1) * sizeof(int) + 64;       // row_idx, pfirst, psecond, col_ptr, bsrc, trl
}

constexpr int kFusedCols = 2;     // columns per level k_solve_fused handles (two-ended chains); wider levels use k_solve_lds

template <bool PROF>
__global__ __launch_bounds__(768) void k_solve_fused(PlanDev pd, StepArgs a) {
    typedef double T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int flags[2];
    __shared__ int lready[kFusedCols];                 // level + 1 whose updated diagonal block is ready in scr
    __shared__ int ntr;
    __shared__ int4 mbuf[3][2];                        // packed level metadata, rolling: levels l, l+1, l+2
    const int tid = threadIdx.x, nth = blockDim.x, wave = tid >> 6, lane = tid & 63, nw = nth >> 6;
    const int n = pd.n, D = pd.D, nnzb = pd.nnzb, nlev = pd.nlev;
    T *Lw = reinterpret_cast<T *>(smem);
    // work region: per-column scratch (updated diagonal block, 36), lazy triples
    T *z = Lw + (size_t)nnzb * 36, *scr = z + D, *zt = scr;
    unsigned short *lazy = reinterpret_cast<unsigned short *>(scr + kFusedCols * 36);
    int *row_idx = reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(scr) + fused_work_bytes(pd, nth)), *pfirst = row_idx + nnzb,
        *psecond = pfirst + nnzb, *col_ptr = psecond + nnzb, *bsrc = col_ptr + n + 1, *trl = bsrc + nnzb;
    const int4 *pmeta = reinterpret_cast<const int4 *>(pd.fz_pmeta);     // [nlev][2]
    // per block: row | col << 8 | shared-y << 24 | pending-y << 25, and its first pending pair
    // src1 | src2 << 15 | count << 30, and the second pair (where chains merge) src1 | src2 << 15
    for (int i = tid; i < nnzb; i += nth) { row_idx[i] = pd.fz_rowinfo[i]; pfirst[i] = pd.fz_pfirst[i]; psecond[i] = pd.fz_psecond[i]; }
    for (int i = tid; i <= n; i += nth) col_ptr[i] = pd.col_ptr[i];
    long long phA = 0, phL = 0, tph = 0, tall = PROF ? clock64() : 0, tload = 0, tsweep = 0, sub[6] = {0, 0, 0, 0, 0, 0}, tsub = 0;
#define BT_SUB(i) do { if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long tq = clock64(); sub[i] += tq - tsub; tsub = tq; } } while (0)
    // (no barrier here: the load of S below does not read these tables; the barrier after it covers both)

    int status = BT_SOLVE_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const double lm = attempt == 0 ? 1e-4 : 1e-3;
        if (tid < 2) flags[tid] = 0;
        if (tid < kFusedCols) lready[tid] = 0;
        // the sweep's tables (their LDS is reused for zt by the back substitution, so a retry reloads them)
        for (int i = tid; i < pd.fz_nlazy; i += nth)          // one 8-byte word per triple: src1, src2, dst | shared << 15
            reinterpret_cast<ushort4 *>(lazy)[i] = make_ushort4((unsigned short)pd.fz_lazy[3 * i], (unsigned short)pd.fz_lazy[3 * i + 1],
                                                               (unsigned short)pd.fz_lazy[3 * i + 2], 0);
        if (tid < 4 && (tid >> 1) < nlev) mbuf[tid >> 1][tid & 1] = pmeta[tid];       // metadata of levels 0 and 1
        lds_load_system_dma<T>(pd, a, Lw, z, bsrc, trl, &ntr, col_ptr, lm, attempt == 0, true, tid, nth);
        __syncthreads();
        if (PROF) tload = clock64() - tall;

        // wave-uniform packed level metadata in SGPRs (ba_plan.cpp: fz_pmeta): current, next and previous level
        int c0a, c0b, c0c, c0d, c1a, c1b, c1c, c1d, n0a = 0, n0b = 0, n0c = 0, n0d = 0, n1a = 0, n1b = 0, n1c = 0, n1d = 0;
        int p0a = 0, p0b = 0, p0c = 0, p1a = 0, p1b = 0, p1c = 0, pnc = 0;
        auto take_next = [&](int l) {
            const int4 m0 = mbuf[l % 3][0], m1 = mbuf[l % 3][1];
            n0a = __builtin_amdgcn_readfirstlane(m0.x); n0b = __builtin_amdgcn_readfirstlane(m0.y);
            n0c = __builtin_amdgcn_readfirstlane(m0.z); n0d = __builtin_amdgcn_readfirstlane(m0.w);
            n1a = __builtin_amdgcn_readfirstlane(m1.x); n1b = __builtin_amdgcn_readfirstlane(m1.y);
            n1c = __builtin_amdgcn_readfirstlane(m1.z); n1d = __builtin_amdgcn_readfirstlane(m1.w);
        };
        take_next(0);
        const bool feeder = tid >= nth - 2;           // the last two threads bring in level l + 2's metadata
        for (int l = 0; l < nlev; ++l) {
            c0a = n0a; c0b = n0b; c0c = n0c; c0d = n0d; c1a = n1a; c1b = n1b; c1c = n1c; c1d = n1d;
            if (PROF) tph = clock64();
            int4 mnext = make_int4(0, 0, 0, 0);
            if (feeder && l + 2 < nlev) mnext = pmeta[(size_t)(l + 2) * 2 + (tid - (nth - 2))];
            const int cnc = (c0b >> 24) & 3;
            const int nr0 = (c0b >> 16) & 255, nr1 = cnc > 1 ? (c1b >> 16) & 255 : 0;     // row waves of the two columns
            const int nA = cnc + nr0 + nr1;                                               // diagonal waves, then row waves
            for (int aw = wave; aw < nA; aw += nw) {
                __builtin_amdgcn_s_setprio(3);
                if (PROF) tsub = clock64();
                if (aw < cnc) {
                    // ---- diagonal wave of column q = aw: bring the diagonal block up to date with its pending
                    // updates (lanes 0..35, one element each) and publish it to the column's row waves
                    const int q = aw, dpos = (q ? c1b : c0b) & 0xffff, md = q ? c1d : c0d;
                    const int el = lane < 36 ? lane : lane - 36, dr = el / 6, dc = el - 6 * dr;
                    const int sd = md & 0x7fff, nd = (md >> 15) & 3;
                    T x[6], yv[6];
                    T v = Lw[(size_t)dpos * 36 + el];
                    load_row6(Lw + (size_t)sd * 36 + 6 * dr, x);
                    load_row6(Lw + (size_t)sd * 36 + 6 * dc, yv);
                    if (nd > 0) {
                        T acc = x[0] * yv[0];
#pragma unroll
                        for (int e = 1; e < 6; ++e) acc += x[e] * yv[e];
                        v -= acc;
                    }
                    if (nd > 1) {                         // where chains merge: a second pending pair (from the level's other column)
                        const T *src = Lw + (size_t)(psecond[dpos] & 0x7fff) * 36;
                        load_row6(src + 6 * dr, x);
                        load_row6(src + 6 * dc, yv);
                        T acc = x[0] * yv[0];
#pragma unroll
                        for (int e = 1; e < 6; ++e) acc += x[e] * yv[e];
                        v -= acc;
                    }
                    if (lane < 36) {
                        scr[q * 36 + lane] = v;
                        Lw[(size_t)dpos * 36 + lane] = v;          // in place as well: its next reader is the back substitution
                    }
                    // the row waves factor it themselves (their own pending update runs meanwhile)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    if (lane == 0) __hip_atomic_store(&lready[q], l + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    BT_SUB(0);
                    __builtin_amdgcn_s_setprio(0);
                } else {
                    // ---- row wave: one panel row (or y_j) per lane: its pending update, then, once the diagonal
                    // wave has published the updated block, its factorisation (every lane, in registers) and the
                    // forward substitution of the row
                    const int ra = aw - cnc, q = ra >= nr0 ? 1 : 0, part = ra - (q ? nr0 : 0);
                    const int ma = q ? c1a : c0a, dpos = (q ? c1b : c0b) & 0xffff;
                    const int j = ma & 255, cnt = (ma >> 8) & 255, ysrc = (ma >> 16) & 255;
                    const int rw = part * 64 + lane;
                    const bool valid = rw <= cnt * 6, isy = rw == cnt * 6;
                    const int sb = rw / 6, r = rw - 6 * sb, bown = dpos + 1 + sb;
                    T *p = isy ? z + 6 * j : Lw + (size_t)bown * 36 + 6 * r;
                    // in[c] -= sum_e avec[e] M[c][e] with avec = row r of src1 and M = src2, or for the y row
                    // avec = y of the source column and M = src1; every load is in flight before the first FMA
                    const unsigned pfo = (unsigned)pfirst[valid && !isy ? bown : dpos];
                    const int s1 = pfo & 0x7fff, s2 = (pfo >> 15) & 0x7fff, no = valid ? (int)(pfo >> 30) : 0;
                    T in[6], avec[6], m[36];
                    load_row6(p, in);
                    load_row6(isy ? z + 6 * ysrc : Lw + (size_t)s1 * 36 + 6 * r, avec);
                    {
                        const T *M = Lw + (size_t)(isy ? s1 : s2) * 36;
#pragma unroll
                        for (int c = 0; c < 6; ++c) load_row6(M + 6 * c, reinterpret_cast<T (&)[6]>(m[6 * c]));
                    }
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
                        T acc = avec[0] * m[6 * c];
#pragma unroll
                        for (int e = 1; e < 6; ++e) acc += avec[e] * m[6 * c + e];
                        in[c] -= no > 0 ? acc : (T)0;
                    }
                    if (__builtin_amdgcn_ballot_w64(no > 1)) {       // where chains merge: a second pending pair
                        const unsigned ps = (unsigned)psecond[isy ? dpos : bown];
                        const int t1 = ps & 0x7fff, t2 = (ps >> 15) & 0x7fff;
                        load_row6(isy ? z + 6 * ((row_idx[t1] >> 8) & 255) : Lw + (size_t)t1 * 36 + 6 * r, avec);
                        const T *M = Lw + (size_t)(isy ? t1 : t2) * 36;
#pragma unroll
                        for (int c = 0; c < 6; ++c) load_row6(M + 6 * c, reinterpret_cast<T (&)[6]>(m[6 * c]));
#pragma unroll
                        for (int c = 0; c < 6; ++c) {
                            T acc = avec[0] * m[6 * c];
#pragma unroll
                            for (int e = 1; e < 6; ++e) acc += avec[e] * m[6 * c + e];
                            in[c] -= no > 1 ? acc : (T)0;
                        }
                    }
                    BT_SUB(3);
                    while (__hip_atomic_load(&lready[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) <= l) __builtin_amdgcn_s_sleep(1);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    T L[21];
                    {
                        const T *dblk = scr + q * 36;
#pragma unroll
                        for (int rr = 0; rr < 6; ++rr) {
                            T row[6];
                            load_row6(dblk + 6 * rr, row);
#pragma unroll
                            for (int c = 0; c <= rr; ++c) L[BT_LT(rr, c)] = row[c];
                        }
                    }
                    const bool ok = chol6_packed<T>(L);
                    if (!ok && part == 0 && lane == 0) flags[0] = 1;
                    BT_SUB(4);
                    if (valid) {
                        T out[6];
#pragma unroll
                        for (int c = 0; c < 6; ++c) {
                            T t = in[c];
#pragma unroll
                            for (int k = 0; k < c; ++k) t -= out[k] * L[BT_LT(c, k)];
                            out[c] = t * L[BT_LT(c, c)];
                        }
                        store_row6(p, out);
                    }
                    BT_SUB(5);
                    __builtin_amdgcn_s_setprio(0);
                }
            }
            if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long tn = clock64(); phA += tn - tph; tph = tn; }
            // ---- lazy updates of the level below: helper waves (all waves once there are more column waves than waves)
            if (l > 0) {
                int h, hs;
                if (nA < nw) { h = tid - 64 * nA; hs = nth - 64 * nA; }
                else { hs = nth; h = (tid + nth - (64 * nA) % nth) % nth; }
                if (h >= 0) {
                    const int rows0 = ((p0c >> 16) & 0xffff) * 6, rows1 = rows0 + (pnc > 1 ? ((p1c >> 16) & 0xffff) * 6 : 0);
                    for (int item = h; item < rows1; item += hs) {
                        const bool sec = item >= rows0;
                        const int idx = item - (sec ? rows0 : 0), t = idx / 6;
                        const ushort4 tr = reinterpret_cast<const ushort4 *>(lazy)[((sec ? p1c : p0c) & 0xffff) + t];
                        apply_update_row3<T>(Lw, tr.x, tr.y, tr.z, idx - 6 * t);
                    }
                    // lazy y contributions of the level below, on the threads after those with update rows
                    {
                        const int ys0 = ((p0a >> 8) & 255) * 6, ys1 = ys0 + (pnc > 1 ? ((p1a >> 8) & 255) * 6 : 0);
                        const int shift = ((rows1 + 63) >> 6) << 6;
                        int first = h - shift;                       // (no division in the usual one-round case)
                        if (shift > hs) first = (h - shift % hs + hs) % hs; else if (first < 0) first += hs;
                        for (int item = first; item < ys1; item += hs) {
                            const bool sec = item >= ys0;
                            const int qq = item - (sec ? ys0 : 0);
                            const int pj = (sec ? p1a : p0a) & 255, dposp = (sec ? p1b : p0b) & 0xffff, sb = qq / 6, r = qq - 6 * sb;
                            const int rcv = row_idx[dposp + 1 + sb];
                            if (rcv & (1 << 25)) continue;            // pending: the destination column's y thread takes it
                            T lr[6], zr[6];
                            load_row6(Lw + (size_t)(dposp + 1 + sb) * 36 + 6 * r, lr);
                            load_row6(z + 6 * pj, zr);
                            T acc = lr[0] * zr[0];
#pragma unroll
                            for (int k = 1; k < 6; ++k) acc += lr[k] * zr[k];
                            lds_sub(z + 6 * (rcv & 255) + r, acc, (rcv & (1 << 24)) != 0);
                        }
                    }
                }
            }
            if (feeder && l + 2 < nlev) mbuf[(l + 2) % 3][tid - (nth - 2)] = mnext;
            if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); phL += clock64() - tph; }
            p0a = c0a; p0b = c0b; p0c = c0c; p1a = c1a; p1b = c1b; p1c = c1c; pnc = cnc;
            if (l + 1 < nlev) take_next(l + 1);
            __syncthreads();
        }
        if (PROF) tsweep = clock64() - tall;

        int4 *bmeta = reinterpret_cast<int4 *>(zt + ((D + 1) & ~1));          // compact level table behind zt
        for (int i = tid; i < nlev * kMaxLevelCols; i += nth) {          // (col, diag pos, #sub-blocks, barrier before this level)
            int4 mm = reinterpret_cast<const int4 *>(pd.fz_meta)[2 * i];
            mm.w = pd.bs_sync[i / kMaxLevelCols];
            bmeta[i] = mm;
        }
        long long tbs[2] = {0, 0};
        lds_back_substitute<T, true>(pd, Lw, z, zt, row_idx, col_ptr, bmeta, 1, tid, nth, PROF ? tbs : nullptr);
        if (PROF) { sub[0] = tbs[0] - tall; sub[1] = tbs[1] - tall; sub[2] = clock64() - tall; }
        for (int i = tid; i < D; i += nth) if (zt[i] != zt[i]) flags[1] = 1;
        __syncthreads();
        const bool failed = flags[0] != 0, has_nan = flags[1] != 0;
        __syncthreads();
        if (failed) {
            for (int i = tid; i < D; i += nth) zt[i] = (T)0;
            status = BT_SOLVE_CHOL_FAILED;
            break;
        }
        if (!has_nan) break;
        status = BT_SOLVE_RETRIED;
    }
    __syncthreads();
    for (int i = tid; i < D; i += nth) a.dx[6 * pd.perm[i / 6] + i % 6] = (float)zt[i];
    if (tid == 0) a.status[0] = status;
    if (PROF && lane == 0) {        // measurement only: per-wave busy cycles (columns, lazy work) and the stage boundaries
        long long *o = reinterpret_cast<long long *>(a.status + 4) + 40 + wave * 2;
        o[0] = phA; o[1] = phL;
        if (wave == 0 || wave == 2) {
            long long *g = reinterpret_cast<long long *>(a.status + 4) + (wave ? 10 : 0);
            g[0] = tload; g[1] = tsweep; g[2] = clock64() - tall;
            for (int i = 0; i < 6; ++i) g[3 + i] = sub[i];       // wave 0: ends of Linv / M form / back substitution; wave 2: row-wave stages
        }
    }
#undef BT_SUB
}

// ------------------------------------------------------------------ k_solve_pipe
// k_solve_fused without the per-level workgroup barrier.  Waves have fixed roles and walk the levels at
// their own pace, ordered by flags in LDS only where data flows:
//   wave q (q = 0, 1)      diagonal wave of the level's column q      -> lready[q]   = level + 1
//   wave 2 + q             row wave of column q (panel rows and y_j)   -> colready[q] = level + 1
//   waves 4 ..             helpers: batch b = the lazy updates whose sources are the columns of level b;
//                          every helper wave adds 1 to hcnt when it has finished its share of a batch
// What a step waits for (tests/plan_emulator.py checks that these waits order every conflicting access):
//   column waves, level l   colready[s] >= l for the columns s of level l - 1 that hold pending sources of this
//                           column (on a chain: its own predecessor only, so the two chains do not wait for
//                           each other) and hcnt >= nh (l - 1): batches 0 .. l - 2 are complete, i.e. every
//                           lazy update into this level's blocks has landed
//   row wave                additionally lready[q] >= l + 1 before it factors
//   helpers, batch b        colready[*] >= b + 1 for the columns of level b (its sources) and
//                           hcnt >= nh b (the whole group has finished the batches before: two batches may
//                           read-modify-write the same destination row from different waves)
// A chain's row wave therefore never waits for anything but its diagonal wave in steady state; the barrier
// (~240 cycles by itself) and the wait for the slowest wave of every level are gone.  Requires columns of at
// most 64 panel rows and levels of at most two columns (plan flag fzp_ok); other systems use k_solve_fused.
__host__ __device__ inline size_t pipe_work_bytes(const PlanDev &pd) {
    const size_t b = 2 * 36 * sizeof(double) + (size_t)pd.fz_nlazy * 4 * sizeof(unsigned short) + 16;
    const size_t zt = (size_t)pd.D * sizeof(double) + (size_t)pd.nlev * kMaxLevelCols * sizeof(int4);   // zt + compact level table
    return ((b > zt ? b : zt) + 15) / 16 * 16;
}
size_t solve_pipe_lds_bytes(const PlanDev &pd) {
    return ((size_t)pd.nnzb * 36 + (size_t)pd.D) * sizeof(double) + pipe_work_bytes(pd) +
           (5 * (size_t)pd.nnzb + (size_t)pd.n + 1 + (size_t)pd.nlev * 8) * sizeof(int) + 64;      // row_idx, pfirst, psecond, col_ptr, level records, bsrc, trl
}


__device__ __forceinline__ void wait_ge(int *flag, int target) {
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
}

template <bool PROF>
__global__ __launch_bounds__(768) void k_solve_pipe(PlanDev pd, StepArgs a) {
    typedef double T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int flags[2];
    __shared__ int lready[2], colready[2], hcnt, ntr;
    const int tid = threadIdx.x, nth = blockDim.x, wave = tid >> 6, lane = tid & 63, nw = nth >> 6;
    const int n = pd.n, D = pd.D, nnzb = pd.nnzb, nlev = pd.nlev;
    T *Lw = reinterpret_cast<T *>(smem);
    T *z = Lw + (size_t)nnzb * 36, *scr = z + D, *zt = scr;
    unsigned short *lazy = reinterpret_cast<unsigned short *>(scr + 2 * 36);
    int *row_idx = reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(scr) + pipe_work_bytes(pd)), *pfirst = row_idx + nnzb,
        *psecond = pfirst + nnzb, *col_ptr = psecond + nnzb, *lrec = col_ptr + n + 1, *bsrc = lrec + nlev * 8, *trl = bsrc + nnzb;
    for (int i = tid; i < nnzb; i += nth) { row_idx[i] = pd.fz_rowinfo[i]; pfirst[i] = pd.fz_pfirst[i]; psecond[i] = pd.fz_psecond[i]; }
    for (int i = tid; i <= n; i += nth) col_ptr[i] = pd.col_ptr[i];
    for (int i = tid; i < nlev * 8; i += nth) lrec[i] = pd.fz_pmeta[i];
    long long tall = PROF ? clock64() : 0, tload = 0, tsweep = 0, twait = 0, twork = 0, tq = 0, sub[3] = {0, 0, 0}, wsplit[2] = {0, 0};
#define BT_TW(acc) do { if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long tn = clock64(); acc += tn - tq; tq = tn; } } while (0)

    int status = BT_SOLVE_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const double lm = attempt == 0 ? 1e-4 : 1e-3;
        if (tid < 2) { flags[tid] = 0; lready[tid] = 0; colready[tid] = 0; }
        if (tid == 2) hcnt = 0;
        for (int i = tid; i < pd.fz_nlazy; i += nth)          // one 8-byte word per triple: src1, src2, dst | shared << 15
            reinterpret_cast<ushort4 *>(lazy)[i] = make_ushort4((unsigned short)pd.fz_lazy[3 * i], (unsigned short)pd.fz_lazy[3 * i + 1],
                                                               (unsigned short)pd.fz_lazy[3 * i + 2], 0);
        lds_load_system_dma<T>(pd, a, Lw, z, bsrc, trl, &ntr, col_ptr, lm, attempt == 0, true, tid, nth);
        __syncthreads();
        if (PROF) { tload = clock64() - tall; tq = clock64(); }

        const int nh = nw - 4;                                   // helper waves
        if (wave < 4) {
            // ================= column waves: q = wave & 1, diagonal wave (wave < 2) or row wave
            const int q = wave & 1;
            const bool is_row = wave >= 2;
            const int4 *lrec4 = reinterpret_cast<const int4 *>(lrec);
            int4 vrec = lrec4[q];                                // this wave's record and slot 0's (it carries the number of columns)
            int vnc = lrec[1];
            int npc = 0;                                         // columns of the level below
            for (int l = 0; l < nlev; ++l) {
                const int ma = __builtin_amdgcn_readfirstlane(vrec.x), mb = __builtin_amdgcn_readfirstlane(vrec.y),
                          md = __builtin_amdgcn_readfirstlane(vrec.w), ncl = (__builtin_amdgcn_readfirstlane(vnc) >> 24) & 3;
                if (l + 1 < nlev) { vrec = lrec4[2 * (l + 1) + q]; vnc = lrec[8 * (l + 1) + 1]; }   // next level's, in flight during this one
                if (q < ncl) {
                    if (l > 0) {
                        // only the columns of the level below that hold pending sources of this column (the record's
                        // dependency bits: on a chain its own predecessor, which this very row wave wrote) and the
                        // helpers' batches; the three flags in one LDS round trip
                        // (the diagonal wave also waits for the row wave that last read its scratch slot)
                        const int dep = ((md >> 20) & 3) | ((!is_row && q < npc) ? 1 << q : 0);
                        const int need0 = (dep & 1) ? l : 0, need1 = (dep & 2) ? l : 0, needh = nh * (l - 1);
                        const long long tw0 = PROF ? clock64() : 0;
                        int lastfail = -1;                           // (PROF: what the wait was for: 1 = the helpers' batch, 0 = a column)
                        for (;;) {
                            const int f0 = __hip_atomic_load(&colready[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            const int f1 = __hip_atomic_load(&colready[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            const int fh = __hip_atomic_load(&hcnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            if (f0 >= need0 && f1 >= need1 && fh >= needh) break;
                            if (PROF) lastfail = fh < needh ? 1 : 0;
                            __builtin_amdgcn_s_sleep(1);
                        }
                        if (PROF && lastfail >= 0) wsplit[lastfail] += clock64() - tw0;
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    }
                    BT_TW(twait);
                    const int dpos = mb & 0xffff;
                    if (!is_row) {
                        // ---- diagonal wave: bring the diagonal block up to date with its pending updates (lanes 0..35,
                        // one element each) and publish it to the row wave
                        const int el = lane < 36 ? lane : lane - 36, dr = el / 6, dc = el - 6 * dr;
                        const int sd = md & 0x7fff, nd = (md >> 15) & 3;
                        T x[6], yv[6];
                        T v = Lw[(size_t)dpos * 36 + el];
                        load_row6(Lw + (size_t)sd * 36 + 6 * dr, x);
                        load_row6(Lw + (size_t)sd * 36 + 6 * dc, yv);
                        if (nd > 0) {
                            T acc = x[0] * yv[0];
#pragma unroll
                            for (int e = 1; e < 6; ++e) acc += x[e] * yv[e];
                            v -= acc;
                        }
                        if (nd > 1) {                         // where chains merge: a second pending pair (from the level's other column)
                            const T *src = Lw + (size_t)(psecond[dpos] & 0x7fff) * 36;
                            load_row6(src + 6 * dr, x);
                            load_row6(src + 6 * dc, yv);
                            T acc = x[0] * yv[0];
#pragma unroll
                            for (int e = 1; e < 6; ++e) acc += x[e] * yv[e];
                            v -= acc;
                        }
                        if (lane < 36) {
                            scr[q * 36 + lane] = v;
                            Lw[(size_t)dpos * 36 + lane] = v;          // in place as well: its next reader is the back substitution
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        if (lane == 0) __hip_atomic_store(&lready[q], l + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        BT_TW(twork);
                    } else {
                        // ---- row wave: one panel row (or y_j) per lane: its pending update, then, once the diagonal wave
                        // has published the updated block, its factorisation (every lane, in registers) and the forward
                        // substitution of the row
                        const int j = ma & 255, cnt = (ma >> 8) & 255, ysrc = (ma >> 16) & 255;
                        const int rw = lane;
                        const bool valid = rw <= cnt * 6, isy = rw == cnt * 6;
                        const int sb = rw / 6, r = rw - 6 * sb, bown = dpos + 1 + sb;
                        T *p = isy ? z + 6 * j : Lw + (size_t)bown * 36 + 6 * r;
                        const unsigned pfo = (unsigned)pfirst[valid && !isy ? bown : dpos];
                        const int s1 = pfo & 0x7fff, s2 = (pfo >> 15) & 0x7fff, no = valid ? (int)(pfo >> 30) : 0;
                        T in[6], avec[6], m[36];
                        load_row6(p, in);
                        load_row6(isy ? z + 6 * ysrc : Lw + (size_t)s1 * 36 + 6 * r, avec);
                        {
                            const T *M = Lw + (size_t)(isy ? s1 : s2) * 36;
#pragma unroll
                            for (int c = 0; c < 6; ++c) load_row6(M + 6 * c, reinterpret_cast<T (&)[6]>(m[6 * c]));
                        }
#pragma unroll
                        for (int c = 0; c < 6; ++c) {
                            T acc = avec[0] * m[6 * c];
#pragma unroll
                            for (int e = 1; e < 6; ++e) acc += avec[e] * m[6 * c + e];
                            in[c] -= no > 0 ? acc : (T)0;
                        }
                        if (__builtin_amdgcn_ballot_w64(no > 1)) {       // where chains merge: a second pending pair
                            const unsigned ps = (unsigned)psecond[isy ? dpos : bown];
                            const int t1 = ps & 0x7fff, t2 = (ps >> 15) & 0x7fff;
                            load_row6(isy ? z + 6 * ((row_idx[t1] >> 8) & 255) : Lw + (size_t)t1 * 36 + 6 * r, avec);
                            const T *M = Lw + (size_t)(isy ? t1 : t2) * 36;
#pragma unroll
                            for (int c = 0; c < 6; ++c) load_row6(M + 6 * c, reinterpret_cast<T (&)[6]>(m[6 * c]));
#pragma unroll
                            for (int c = 0; c < 6; ++c) {
                                T acc = avec[0] * m[6 * c];
#pragma unroll
                                for (int e = 1; e < 6; ++e) acc += avec[e] * m[6 * c + e];
                                in[c] -= no > 1 ? acc : (T)0;
                            }
                        }
                        BT_TW(sub[0]);
                        wait_ge(&lready[q], l + 1);
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                        BT_TW(sub[1]);
                        T L[21];
                        {
                            const T *dblk = scr + q * 36;
#pragma unroll
                            for (int rr = 0; rr < 6; ++rr) {
                                T row[6];
                                load_row6(dblk + 6 * rr, row);
#pragma unroll
                                for (int c = 0; c <= rr; ++c) L[BT_LT(rr, c)] = row[c];
                            }
                        }
                        const bool ok = chol6_packed<T>(L);
                        // (substitution computed by every lane, only the store is predicated: one basic block, so the
                        //  compiler can slot its FMAs into the latency gaps of the factorisation)
                        T out[6];
#pragma unroll
                        for (int c = 0; c < 6; ++c) {
                            T t = in[c];
#pragma unroll
                            for (int k = 0; k < c; ++k) t -= out[k] * L[BT_LT(c, k)];
                            out[c] = t * L[BT_LT(c, c)];
                        }
                        if (valid) store_row6(p, out);
                        if (!ok && lane == 0) flags[0] = 1;
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        if (lane == 0) __hip_atomic_store(&colready[q], l + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        BT_TW(sub[2]);
                    }
                }
                npc = ncl;
            }
        } else {
            // ================= helper waves: batch b = lazy updates and lazy y contributions of the columns of level b
            const int h = tid - 256, hs = nth - 256;
            for (int b = 0; b + 1 < nlev; ++b) {
                const int p0a = __builtin_amdgcn_readfirstlane(lrec[8 * b]), p0b = __builtin_amdgcn_readfirstlane(lrec[8 * b + 1]),
                          p0c = __builtin_amdgcn_readfirstlane(lrec[8 * b + 2]), p1a = __builtin_amdgcn_readfirstlane(lrec[8 * b + 4]),
                          p1b = __builtin_amdgcn_readfirstlane(lrec[8 * b + 5]), p1c = __builtin_amdgcn_readfirstlane(lrec[8 * b + 6]);
                const int pnc = (p0b >> 24) & 3;
                {
                    const int need1 = pnc > 1 ? b + 1 : 0;
                    for (;;) {
                        const int f0 = __hip_atomic_load(&colready[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        const int f1 = __hip_atomic_load(&colready[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        const int fh = __hip_atomic_load(&hcnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (f0 >= b + 1 && f1 >= need1 && fh >= nh * b) break;
                        __builtin_amdgcn_s_sleep(1);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                BT_TW(twait);
                const int rows0 = ((p0c >> 16) & 0xffff) * 6, rows1 = rows0 + (pnc > 1 ? ((p1c >> 16) & 0xffff) * 6 : 0);
                for (int item = h; item < rows1; item += hs) {
                    const bool sec = item >= rows0;
                    const int idx = item - (sec ? rows0 : 0), t = idx / 6;
                    const ushort4 tr = reinterpret_cast<const ushort4 *>(lazy)[((sec ? p1c : p0c) & 0xffff) + t];
                    apply_update_row3<T>(Lw, tr.x, tr.y, tr.z, idx - 6 * t);
                }
                {
                    const int ys0 = ((p0a >> 8) & 255) * 6, ys1 = ys0 + (pnc > 1 ? ((p1a >> 8) & 255) * 6 : 0);
                    const int shift = ((rows1 + 63) >> 6) << 6;
                    int first = h - shift;                       // (no division in the usual one-round case)
                    if (shift > hs) first = (h - shift % hs + hs) % hs; else if (first < 0) first += hs;
                    for (int item = first; item < ys1; item += hs) {
                        const bool sec = item >= ys0;
                        const int qq = item - (sec ? ys0 : 0);
                        const int pj = (sec ? p1a : p0a) & 255, dposp = (sec ? p1b : p0b) & 0xffff, sb = qq / 6, r = qq - 6 * sb;
                        const int rcv = row_idx[dposp + 1 + sb];
                        if (rcv & (1 << 25)) continue;            // pending: the destination column's y thread takes it
                        T lr[6], zr[6];
                        load_row6(Lw + (size_t)(dposp + 1 + sb) * 36 + 6 * r, lr);
                        load_row6(z + 6 * pj, zr);
                        T acc = lr[0] * zr[0];
#pragma unroll
                        for (int k = 1; k < 6; ++k) acc += lr[k] * zr[k];
                        lds_sub(z + 6 * (rcv & 255) + r, acc, (rcv & (1 << 24)) != 0);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if (lane == 0) __hip_atomic_fetch_add(&hcnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                BT_TW(twork);
            }
        }
        __syncthreads();
        if (PROF) tsweep = clock64() - tall;

        int4 *bmeta = reinterpret_cast<int4 *>(zt + ((D + 1) & ~1));          // compact level table behind zt
        for (int i = tid; i < nlev * kMaxLevelCols; i += nth) {          // (col, diag pos, #sub-blocks, barrier before this level)
            int4 mm = reinterpret_cast<const int4 *>(pd.fz_meta)[2 * i];
            mm.w = pd.bs_sync[i / kMaxLevelCols];
            bmeta[i] = mm;
        }
        lds_back_substitute<T, true>(pd, Lw, z, zt, row_idx, col_ptr, bmeta, 1, tid, nth, nullptr);
        for (int i = tid; i < D; i += nth) if (zt[i] != zt[i]) flags[1] = 1;
        __syncthreads();
        const bool failed = flags[0] != 0, has_nan = flags[1] != 0;
        __syncthreads();
        if (failed) {
            for (int i = tid; i < D; i += nth) zt[i] = (T)0;
            status = BT_SOLVE_CHOL_FAILED;
            break;
        }
        if (!has_nan) break;
        status = BT_SOLVE_RETRIED;
    }
    __syncthreads();
    for (int i = tid; i < D; i += nth) a.dx[6 * pd.perm[i / 6] + i % 6] = (float)zt[i];
    if (tid == 0) a.status[0] = status;
    if (PROF && lane == 0) {        // measurement only: per-wave (waiting, working) cycles of the sweep
        long long *o = reinterpret_cast<long long *>(a.status + 4) + 40 + wave * 2;
        o[0] = twait; o[1] = twork + sub[0] + sub[2];
        if (wave == 0 || wave == 2) {
            long long *g = reinterpret_cast<long long *>(a.status + 4) + (wave ? 10 : 0);
            g[0] = tload; g[1] = tsweep; g[2] = clock64() - tall;
            g[3] = sub[0]; g[4] = sub[1]; g[5] = sub[2]; g[6] = twait; g[7] = wsplit[0]; g[8] = wsplit[1];
        }
    }
#undef BT_TW
}


// ------------------------------------------------------------------ refinement of float32-factor solves
// Systems whose factor does not fit LDS as double are factored in float32 (k_solve_lds<float>, k_solve_global): dX is then
// 5e-5 .. 1e-4 off the exact solution of [S | y] — outside the parity contract.  Iterative refinement, only for those systems:
// r = y - A dX0 in double from the S still in global memory (A = S + (ep + lm S) I, ba.py:67, with the lm the first solve
// ended on), the same solver once more on r, dX = dX0 + delta — TWICE (kRefineSteps): a step shrinks the error by
// cond(A) * 6e-8 * a small constant, and the 100-300-pose graphs that land here reach cond(A) = 3e5 with ep = 10, where one
// step left dX 9.4e-6 and the pose update 1.1e-5 from the float64 solve (tests/gpu_seed_probe.py, seed 32862) — outside the
// 1e-5 of the contract; two leave it at the float32 rounding of dX.  y holds the current residual throughout
// (r_{p+1} = r_p - A delta_p), dx0 the sum so far.  A failed factorisation gives 0 + 0 + 0 (ba.py:9-13).
// The second step is skipped where the first already converged: a step's correction is the error before it, the error after it
// that correction times the same contraction rho = |delta_1| / |dX0| — so |delta_1| <= 1.5e-4 |dX0| means the sum is within
// 2.3e-8 of the float64 solve, the float32 rounding of dX.  The residual kernel of the second step raises kRefineDone, the solve
// behind it returns at once and k_refine_add takes the sum as it is (a well-conditioned band pays two solves, not three).
constexpr int kRefineSteps = 2;
__global__ __launch_bounds__(256) void k_refine_residual(PlanDev pd, StepArgs a, int accumulate) {
    const int D = pd.D, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + w;
    if (i >= D) return;
    const double lm = a.status[0] == BT_SOLVE_RETRIED ? 1e-3 : 1e-4;
    double acc = 0.0;
    for (int j = lane; j < D; j += 64) {
        double s = i >= j ? a.S[(size_t)i * D + j] : a.S[(size_t)j * D + i];            // S holds the lower triangle
        if (i == j) s = s + ((double)a.ep + lm * s);
        acc += s * (double)a.dx[j];
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) a.y[i] = a.y[i] - acc;
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        double nd = 0.0, nx = 0.0;
        for (int k = threadIdx.x; k < D; k += 64) {
            const float d = a.dx[k], x = accumulate ? a.dx0[k] : 0.0f;
            nd += (double)d * d; nx += (double)x * x;
            a.dx0[k] = accumulate ? x + d : d;
        }
        for (int o = 32; o > 0; o >>= 1) { nd += __shfl_xor(nd, o); nx += __shfl_xor(nx, o); }
        if (threadIdx.x == 0) a.status[kRefineDone] = (accumulate && nd <= 2.25e-8 * nx) ? 1 : 0;      // (NaN: not done)
    }
}

// (one workgroup: it reads the flag, and clears it for the next step's first solve when everybody has)
__global__ __launch_bounds__(1024) void k_refine_add(PlanDev pd, StepArgs a) {
    const bool done = a.status[kRefineDone] != 0;
    for (int k = threadIdx.x; k < pd.D; k += blockDim.x) a.dx[k] = done ? a.dx0[k] : a.dx0[k] + a.dx[k];
    __syncthreads();
    if (threadIdx.x == 0) a.status[kRefineDone] = 0;
}

// ------------------------------------------------------------------ k_update
// One BA step's last kernel.  Block ranges (512 threads each):
//   [0, tile_blocks)         pose+structure steps only: one block per tile of tracks.  The depth update
//                            dZ_k = Q_k (w'_k - sum_c E[c,k]^T dX_c) (ba.py:328) is evaluated WITHOUT a stored E:
//                            E[c,k]^T dX_c summed over the cameras of a track is, edge by edge,
//                            Jz^T W (Jj dX_j + Ji dX_i) = Jz^T W Jj (dX_j - Ad(Gij) dX_i)  (Ji = -Jj Ad, projective_ops.py:96),
//                            so the block forms delta = dX_j - Ad dX_i once per camera pair of the tile (from the
//                            pair geometry k_tile left in the workspace) and re-evaluates the edge Jacobians from
//                            targets / weights: 16 B per edge read again instead of 24 B per edge written and read back.
//   [.., + patch_blocks)     the whole patch buffer: copy of x, y and the clamp of ba.py:333; structure-only steps
//                            add dZ = Q w' (ba.py:316-317) here; pose+structure steps skip the patches that carry
//                            a track (the tile blocks write those).  Followed by one thread per buffer pose:
//                            Exp(dX) * G in double (groups.py:153-156).
//   [first_zero_block, ..)   [S | y] has been consumed by the solver: cleared for the next step's accumulation.
constexpr int kUpdThreads = 512;
constexpr int kUpdGeo = 28;          // floats per pair in LDS: the 20 of kPairGeomFloats, delta (6), padding to 16 bytes

// THREADS: 512, or 1024 for the few-tiles / many-slots graphs that k_tile runs 16 waves wide (tile_wide): the tile blocks'
// slot loop, which is all the time there is on 40 tiles, halves.
template <bool SO, int THREADS = kUpdThreads, typename R = float>
__global__ __launch_bounds__(THREADS) void k_update(PlanDev pd, StepArgs a, int do_poses, int tile_blocks, int first_zero_block) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    R *lds = reinterpret_cast<R *>(lds_raw);
    typedef typename Vec2<R>::type R2;
    if (!SO && (int)blockIdx.x >= first_zero_block) {
        const size_t nz = (size_t)pd.D * pd.D + pd.D;
        const size_t i0 = ((size_t)(blockIdx.x - first_zero_block) * blockDim.x + threadIdx.x) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (i0 + k < nz) a.S[i0 + k] = 0.0;
        return;
    }
    if (!SO && (int)blockIdx.x < tile_blocks) {
        // (an XCD's workgroups take a contiguous range of tiles, as in k_tile)
        const int tq_ = tile_blocks >> 3, tr_ = tile_blocks & 7, xcd_ = blockIdx.x & 7;
        const int tile = xcd_ * tq_ + min(xcd_, tr_) + ((int)blockIdx.x >> 3), tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
        constexpr int kWaves = THREADS / 64;
        R *geo = lds;                                               // [npair][kUpdGeo]
        R *part = lds + (size_t)pd.max_tile_pairs * kUpdGeo;        // [kWaves][64]
        const int np = pd.tile_npair[tile];
        const int patch = pd.tile_kx[(size_t)tile * kLanes + lane];
        const int slot0 = pd.tile_slot0[tile], nslot = pd.tile_nslot[tile];
        const int chunk = (nslot + kWaves - 1) / kWaves;
        const int s0 = wave * chunk, s1 = min(nslot, s0 + chunk);
        int e_nx = -1, lp_nx = 0;
        if (s0 < s1) { const size_t idx = (size_t)(slot0 + s0) * kLanes + lane; e_nx = pd.slot_edge[idx]; lp_nx = pd.slot_lp[idx]; }
        for (int p = tid; p < np; p += THREADS) {
            const int gp = pd.tile_pairs[pd.tile_pair0[tile] + p];
            const int ia = pd.pair_i[gp] - pd.fixedp, ib = pd.pair_j[gp] - pd.fixedp;
            R g[kPairGeomFloats];
            const R2 *src = reinterpret_cast<const R2 *>(reinterpret_cast<const R *>(a.pairgeo) + (size_t)gp * kPairGeomFloats);
#pragma unroll
            for (int c = 0; c < kPairGeomFloats / 2; ++c) { const R2 t2 = src[c]; g[2*c] = t2.x; g[2*c + 1] = t2.y; }
            R xi[6] = {0, 0, 0, 0, 0, 0}, xj[6] = {0, 0, 0, 0, 0, 0};
            if (ia >= 0) for (int c = 0; c < 6; ++c) xi[c] = a.dx[6 * ia + c];
            if (ib >= 0) for (int c = 0; c < 6; ++c) xj[c] = a.dx[6 * ib + c];
            // Ad(Gij) (tau, phi) = (R tau + t x (R phi), R phi)        (se3.h:58-67)
            R Rt[3], Rp[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                Rt[r] = g[3*r] * xi[0] + g[3*r + 1] * xi[1] + g[3*r + 2] * xi[2];
                Rp[r] = g[3*r] * xi[3] + g[3*r + 1] * xi[4] + g[3*r + 2] * xi[5];
            }
            R *o = geo + (size_t)p * kUpdGeo;
#pragma unroll
            for (int c = 0; c < kPairGeomFloats; ++c) o[c] = g[c];
            o[20] = xj[0] - (Rt[0] + g[10] * Rp[2] - g[11] * Rp[1]);
            o[21] = xj[1] - (Rt[1] + g[11] * Rp[0] - g[9]  * Rp[2]);
            o[22] = xj[2] - (Rt[2] + g[9]  * Rp[1] - g[10] * Rp[0]);
            o[23] = xj[3] - Rp[0]; o[24] = xj[4] - Rp[1]; o[25] = xj[5] - Rp[2];
            o[26] = (R)0; o[27] = (R)0;
        }
        R px = 0, py = 0, pdisp = 0;
        if (patch >= 0) { px = a.patches[3*patch]; py = a.patches[3*patch + 1]; pdisp = a.patches[3*patch + 2]; }
        R tu_nx = 0, tv_nx = 0, w0_nx = 0, w1_nx = 0;
        if (e_nx >= 0) {
            const float *tp = a.targets + (size_t)e_nx * a.tstride;
            tu_nx = tp[0]; tv_nx = tp[1];
            const float2 w = reinterpret_cast<const float2 *>(a.weights)[e_nx];
            w0_nx = w.x; w1_nx = w.y;
        }
        __syncthreads();
        R acc = 0;
#pragma unroll 1
        for (int s = s0; s < s1; ++s) {
            const int e = e_nx, lp = lp_nx;
            const R tu = tu_nx, tv = tv_nx, w0 = w0_nx, w1 = w1_nx;
            if (s + 1 < s1) {
                const size_t idn = (size_t)(slot0 + s + 1) * kLanes + lane;
                e_nx = pd.slot_edge[idn]; lp_nx = pd.slot_lp[idn];
                tu_nx = tv_nx = w0_nx = w1_nx = (R)0;
                if (e_nx >= 0) {
                    const float *tp = a.targets + (size_t)e_nx * a.tstride;
                    tu_nx = tp[0]; tv_nx = tp[1];
                    const float2 w = reinterpret_cast<const float2 *>(a.weights)[e_nx];
                    w0_nx = w.x; w1_nx = w.y;
                }
            }
            R g[kUpdGeo];
            if (sizeof(R) == 4) {
                const float4 *g4 = reinterpret_cast<const float4 *>(geo + (size_t)lp * kUpdGeo);
#pragma unroll
                for (int c = 0; c < kUpdGeo / 4; ++c) { const float4 t4 = g4[c]; g[4*c] = t4.x; g[4*c + 1] = t4.y; g[4*c + 2] = t4.z; g[4*c + 3] = t4.w; }
            } else {
                const double2 *g2 = reinterpret_cast<const double2 *>(geo + (size_t)lp * kUpdGeo);
#pragma unroll
                for (int c = 0; c < kUpdGeo / 2; ++c) { const double2 t2 = g2[c]; g[2*c] = t2.x; g[2*c + 1] = t2.y; }
            }
            EdgeQT<R> q;
            edge_eval<R>(g, px, py, pdisp, tu, tv, w0, w1, a, q);
            if (e < 0) continue;
            const R d0 = q.a0 * g[20] + q.a2 * g[22] + q.a3 * g[23] + q.a4 * g[24] + q.a5 * g[25];
            const R d1 = q.b1 * g[21] + q.b2 * g[22] + q.b3 * g[23] + q.b4 * g[24] + q.b5 * g[25];
            acc += q.W0 * q.jz0 * d0 + q.W1 * q.jz1 * d1;
        }
        part[wave * 64 + lane] = acc;
        __syncthreads();
        if (wave == 0 && patch >= 0) {
            R tot = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) tot += part[w * 64 + lane];
            const R2 qw = reinterpret_cast<const R2 *>(a.qw)[pd.tile_trk0[tile] + lane];
            float dd = (float)(pdisp + qw.x * (qw.y - tot));                // ba.py:328, :333
            dd = dd < 1e-3f ? 1e-3f : dd;
            dd = dd > 10.0f ? 10.0f : dd;
            a.patches_out[3*patch] = (float)px; a.patches_out[3*patch + 1] = (float)py; a.patches_out[3*patch + 2] = dd;
        }
        return;
    }
    update_rest<SO, !SO>(pd, a, (int)(blockIdx.x - (SO ? 0 : tile_blocks)) * (int)blockDim.x + (int)threadIdx.x, do_poses);
}

// ------------------------------------------------------------------ k_pack_system
// Dense [S | y] (caller order, lower triangle) <-> the plan's non-zero blocks in factor order followed by
// y in factor order: the multi-GPU exchange buffer (include/batrack_ba.h: bt_ba_pack).  One thread per element.
// block b of a WIDE plan's packed form (ba_plan.cpp: no symbolic factorisation, every lower block): b = rn (rn + 1) / 2 + cn
__device__ __forceinline__ void wide_block(int b, int &rn, int &cn) {
    rn = (int)((sqrtf(8.0f * (float)b + 1.0f) - 1.0f) * 0.5f);
    while ((rn + 1) * (rn + 2) / 2 <= b) ++rn;
    while (rn * (rn + 1) / 2 > b) --rn;
    cn = b - rn * (rn + 1) / 2;
}

template <bool UNPACK>
__global__ __launch_bounds__(256) void k_pack_system(PlanDev pd, StepArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, nb = pd.nnzb * 36;
    if (pd.wide) {
        if (i < nb) {
            const int b = i / 36, e = i - 36 * b, r = e / 6, c = e - 6 * r;
            int rn, cn;
            wide_block(b, rn, cn);
            if (rn == cn && c > r) { if (!UNPACK) a.packed[i] = 0.0; return; }
            double *p = a.S + (size_t)(6 * rn + r) * pd.D + 6 * cn + c;
            if (UNPACK) *p = a.packed[i]; else a.packed[i] = *p;
        } else if (i < nb + pd.D) {
            if (UNPACK) a.y[i - nb] = a.packed[i]; else a.packed[i] = a.y[i - nb];
        }
        return;
    }
    if (i < nb) {
        const int b = i / 36, e = i - 36 * b, r = e / 6, c = e - 6 * r, src = pd.blk_src[b];
        const int rn = src >> 9, cn = (src >> 1) & 255;
        const bool diag = rn == cn;
        if (diag && c > r) { if (!UNPACK) a.packed[i] = 0.0; return; }       // S holds the lower triangle only
        double *p = (src & 1) ? a.S + (size_t)(6 * rn + c) * pd.D + 6 * cn + r : a.S + (size_t)(6 * rn + r) * pd.D + 6 * cn + c;
        if (UNPACK) *p = a.packed[i]; else a.packed[i] = *p;
    } else if (i < nb + pd.D) {
        const int k = i - nb;
        double *p = a.y + 6 * pd.perm[k / 6] + k % 6;
        if (UNPACK) *p = a.packed[i]; else a.packed[i] = *p;
    }
}

// ------------------------------------------------------------------ one-shot exchange of [S | y] between the ranks' GPUs
// The reduced system in its packed form is ~140 KB at 64 keyframes, ~33 KB for the 15-pose window: an all-reduce of that
// size is pure latency, and xGMI is a full mesh of point-to-point links — so every rank WRITES its packed partial system
// straight into a slot of every peer's exchange buffer (hipIpc-mapped, uncached device memory) and raises a flag there;
// every rank then sums the `world` slots of its own buffer in rank order (bitwise the same sum everywhere, so every rank
// solves the identical system) while unpacking into [S | y].  No collective library, no host round trip, nothing but two
// kernels on the compute stream.  Buffer layout (bt_xchg_bytes): [2 parities][world slots][slot doubles] | flags [2][world]
// int64 | a ticket counter.  Epoch e uses parity e & 1: a rank cannot start epoch e + 2 before it has seen every peer's flag
// of epoch e + 1, which a peer raises only after it has consumed epoch e.
__device__ __forceinline__ double *packed_elem(const PlanDev &pd, const StepArgs &a, int i, bool &zero) {
    const int nb = pd.nnzb * 36;
    zero = false;
    if (pd.wide) {
        if (i >= nb) return a.y + (i - nb);
        const int b = i / 36, e = i - 36 * b, r = e / 6, c = e - 6 * r;
        int rn, cn;
        wide_block(b, rn, cn);
        if (rn == cn && c > r) { zero = true; return nullptr; }
        return a.S + (size_t)(6 * rn + r) * pd.D + 6 * cn + c;
    }
    if (i < nb) {
        const int b = i / 36, e = i - 36 * b, r = e / 6, c = e - 6 * r, src = pd.blk_src[b];
        const int rn = src >> 9, cn = (src >> 1) & 255;
        if (rn == cn && c > r) { zero = true; return nullptr; }              // S holds the lower triangle only
        return (src & 1) ? a.S + (size_t)(6 * rn + c) * pd.D + 6 * cn + r : a.S + (size_t)(6 * rn + r) * pd.D + 6 * cn + c;
    }
    const int k = i - nb;
    return a.y + 6 * pd.perm[k / 6] + k % 6;
}

struct XchgPeers { double *buf[kMaxRanks]; };

__device__ __forceinline__ size_t xchg_slot_doubles(const PlanDev &pd) { return ((size_t)pd.nnzb * 36 + pd.D + 1) & ~(size_t)1; }

__global__ __launch_bounds__(256) void k_xchg_push(PlanDev pd, StepArgs a, XchgPeers peers, int world, int rank, long long epoch) {
    const int total = pd.nnzb * 36 + pd.D;
    const size_t slot = xchg_slot_doubles(pd), off = ((size_t)(epoch & 1) * world + rank) * slot;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        bool zero;
        double *p = packed_elem(pd, a, i, zero);
        const double v = zero ? 0.0 : *p;
        for (int q = 0; q < world; ++q) __builtin_nontemporal_store(v, peers.buf[q] + off + i);
    }
    // every block: its stores out to the fabric, then a ticket; the last block raises this rank's flag in every peer's buffer
    __threadfence_system();
    __syncthreads();
    __shared__ int last;
    long long *own_flags = reinterpret_cast<long long *>(peers.buf[rank] + 2 * (size_t)world * slot);
    int *ticket = reinterpret_cast<int *>(own_flags + 2 * world);
    if (threadIdx.x == 0) last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence_system();
    if ((int)threadIdx.x < world) {
        long long *f = reinterpret_cast<long long *>(peers.buf[threadIdx.x] + 2 * (size_t)world * slot) + (size_t)(epoch & 1) * world + rank;
        __hip_atomic_store(f, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Waits for the flags of epoch `epoch` from all ranks, then [S | y] = sum over the ranks' slots, in rank order.  The wait is
// bounded (a peer that never arrives must not hang the GPU).  A time-out is FATAL for the step, never a silent wrong answer:
// status word 1 is set to BT_XCHG_TIMEOUT (sticky until bt_ba_workspace_init), and the last block to finish plants a
// non-positive pivot in S, so that the solver that follows reports a failed factorisation and the step leaves the poses
// where they were (dX = 0, the reference's own reaction to a failed Cholesky, ba.py:9-13) instead of solving a partial system;
// the depths then move by their rank-local Q w' only.  The caller polls bt_ba_xchg_status and raises (parallel.py).
__global__ __launch_bounds__(256) void k_xchg_pull(PlanDev pd, StepArgs a, double *own, int world, long long epoch, long long spin_limit) {
    const size_t slot = xchg_slot_doubles(pd);
    const long long *flags = reinterpret_cast<const long long *>(own + 2 * (size_t)world * slot) + (size_t)(epoch & 1) * world;
    if ((int)threadIdx.x < world) {
        long long it = 0;
        while (__hip_atomic_load(flags + threadIdx.x, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < epoch) {
            __builtin_amdgcn_s_sleep(8);
            if (++it > spin_limit) { __hip_atomic_store(a.status + 1, (int)BT_XCHG_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
        }
    }
    __syncthreads();
    __threadfence_system();
    const int total = pd.nnzb * 36 + pd.D;
    const double *base = own + (size_t)(epoch & 1) * world * slot;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        bool zero;
        double *p = packed_elem(pd, a, i, zero);
        if (zero) continue;
        double v = 0.0;
        for (int q = 0; q < world; ++q) v += __builtin_nontemporal_load(base + (size_t)q * slot + i);
        *p = v;
    }
    // the last block (a ticket in the rank's own buffer: the push of this step left it at 0) checks the verdict of ALL blocks
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        long long *own_flags = reinterpret_cast<long long *>(own + 2 * (size_t)world * slot);
        int *ticket = reinterpret_cast<int *>(own_flags + 2 * world) + 1;
        if (__hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1) {
            __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__hip_atomic_load(a.status + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)BT_XCHG_TIMEOUT)
                for (int d = 0; d < pd.D; ++d) a.S[(size_t)d * pd.D + d] = -1e300;      // every pivot fails whatever the elimination order
        }
    }
}

size_t xchg_bytes(const PlanDev &pd, int world) {
    const size_t slot = (((size_t)pd.nnzb * 36 + pd.D + 1) & ~(size_t)1) * sizeof(double);
    return 2 * (size_t)world * slot + 2 * (size_t)world * sizeof(long long) + 64;
}

int launch_xchg_push(const PlanDev &pd, const StepArgs &a, void *const *bufs, int world, int rank, long long epoch, hipStream_t st) {
    const int total = pd.nnzb * 36 + pd.D;
    if (total <= 0) return BT_OK;
    XchgPeers P{};
    for (int q = 0; q < world; ++q) P.buf[q] = static_cast<double *>(bufs[q]);
    const int nb = std::min(64, (total + 255) / 256);
    hipLaunchKernelGGL(k_xchg_push, dim3(nb), dim3(256), 0, st, pd, a, P, world, rank, epoch);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

int launch_xchg_pull(const PlanDev &pd, const StepArgs &a, void *own, int world, long long epoch, hipStream_t st) {
    const int total = pd.nnzb * 36 + pd.D;
    if (total <= 0) return BT_OK;
    static const long long limit = std::getenv("BT_XCHG_SPIN_LIMIT") ? std::atoll(std::getenv("BT_XCHG_SPIN_LIMIT")) : 20000000ll;   // tens of seconds of polls (each an uncached load + s_sleep): first-launch code loading and host stalls must not trip it
    const int nb = std::min(64, (total + 255) / 256);
    hipLaunchKernelGGL(k_xchg_pull, dim3(nb), dim3(256), 0, st, pd, a, static_cast<double *>(own), world, epoch, limit);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

// ------------------------------------------------------------------ the plan's route
// rsz: sizeof(R) of the k_tile instantiation
static inline size_t tile_lds_bytes_r(const PlanDev &pd, bool so, size_t rsz, size_t kTileWaves) {
    const size_t rows = so ? 0 : (size_t)pd.max_rows16;
    const size_t mtp = pd.max_tile_pairs > 0 ? (size_t)pd.max_tile_pairs : 1;
    return (rows * kLdsRowStride + kTileWaves * 8 * 64 + 128 + mtp * kPairGeomFloats) * rsz + (kTileWaves * 64 + rows) * sizeof(int) + 64;
}

// 12 waves: enough helper threads for one round of update rows on banded systems, and a 170-register budget per thread so
// that a whole 6x6 operand block can be in flight from LDS
constexpr int kSolveThreads = 768;

// Which kernels the plan's steps launch: from the plan's scalars and BT_FORCE (tests, measurement) alone, once per plan.
static Route plan_route(const PlanDev &pd) {
    const Force &f = force();
    Route r{};
    // Jacobian kernel.  k_edge2 / k_edge2u take graphs of many tiles, all slot-uniform (the plan's em_ok), whose tiles see at
    // most 10 cameras (row tiles of the Schur product) and 64 camera pairs (one lane per pair in the prologue); k_stream those
    // whose tiles see at most 10 cameras (row tiles of its register accumulators) and 32 camera pairs (one lane per pair in the
    // prologue, LDS of the per-pair sums).  The plan records the tile counts it was laid out for (em_min, st_min).
    // Measured on the benchmark generator (whole-step times; profiles/r02_kernel_choice.txt, r05_edge2_vs_edge.txt): k_tile is
    // fastest up to ~1500 tiles; from 2048 tiles k_edge2 where the tiles are slot-uniform (whole step 122 against k_stream's 130 us
    // at 2048 tiles, 151 against 160 at 4096), k_stream otherwise (tiles of more than 64 slots: the edge-major layout does not
    // hold them).  The pair-major k_etile takes the graphs k_tile would take that were tiled for it (pm_ok 2) when the tile's
    // E fits LDS as double.
    if (pd.T > 0 && pd.em_ok && pd.T >= pd.em_min && pd.max_cams <= 10 && pd.max_cams > 0 && pd.max_tile_pairs <= 64 && pd.max_tile_pairs > 0)
        r.kernel = Route::kEdge;
    else if (pd.T > 0 && pd.st_ok && pd.T >= pd.st_min && pd.max_cams <= 10 && pd.max_tile_pairs <= 32 && pd.max_tile_pairs > 0)
        r.kernel = Route::kStream;
    else if (pd.T > 0 && pd.pm_ok == 2 && etile_full_lds_bytes(pd.max_rows16, pd.max_tile_pairs, sizeof(double)) <= kEtileLdsBudget)
        r.kernel = Route::kEtile;
    else
        r.kernel = Route::kTile;
    // per-edge maths: mixed on the wave-per-tile kernels (ba_edge.hpp: edge_eval_mixed); float64 on k_etile, and on k_tile where
    // its 8-wave tile fits LDS as double; float32 on request (BT_FORCE prec=f32)
    if (r.kernel == Route::kEdge || r.kernel == Route::kStream) r.prec = 6;
    else if (f.f32_edges || pd.T <= 0) r.prec = 4;
    else r.prec = r.kernel == Route::kEtile || tile_lds_bytes_r(pd, false, sizeof(double), 8) <= kLdsBudget ? 8 : 4;
    // k_tile runs 16 waves per tile on graphs of few tiles with deep slot loops (BT_FORCE wide=0 / wide=1 forces: measurement
    // only).  The float64 instantiation runs 8 waves whatever the graph: its slot loop wants more than the 128 registers a
    // 16-wave workgroup leaves a thread, and the window graphs' SIMDs are issue-saturated at 8 waves already.
    r.wide = r.kernel == Route::kTile && r.prec == 4 && (f.tile_wide >= 0 ? f.tile_wide != 0 : pd.T <= 128 && pd.max_tile_slots >= 24);
    // reduced solver: dense for wide plans (more than 255 free poses, or a factor too large for LDS as double: ba_dense.hip);
    // else the factor in LDS as double where it fits, as float where that fits, else in the global workspace (both float ones
    // refined).  Of the double ones: the barrier-free k_solve_pipe where the schedule allows it, else k_solve_fused (one
    // workgroup barrier per level), else the two-phase k_solve_lds.  BT_FORCE solver=fused | lds | lds32 | global.
    const int fs = f.solver;
    if (pd.wide) r.solver = Route::kSolveDense;
    else if (fs == 3) r.solver = Route::kSolveGlobal;
    else if (fs == 2 && solve_lds_bytes(pd, sizeof(float)) <= kLdsBudget) r.solver = Route::kSolveLds32;
    else if (solve_lds_bytes(pd, sizeof(double)) <= kLdsBudget) {
        if (fs < 0 && pd.fzp_ok && pd.fz_ok && solve_pipe_lds_bytes(pd) <= kLdsBudget) r.solver = Route::kSolvePipe;
        else if (fs != 1 && pd.fz_ok && solve_fused_lds_bytes(pd, kSolveThreads) <= kLdsBudget) r.solver = Route::kSolveFused;
        else r.solver = Route::kSolveLds;
    }
    else if (solve_lds_bytes(pd, sizeof(float)) <= kLdsBudget) r.solver = Route::kSolveLds32;
    else r.solver = Route::kSolveGlobal;
    return r;
}

// ------------------------------------------------------------------ launchers
// The k_tile (K = 1), solver (K = 3) or k_update (K = 4) instantiation of a route, its workgroup and dynamic LDS, and the LDS
// limit kept for it (K: the kernel numbers of the event pairs below).  fn == nullptr: the route launches none of that family
// (k_stream, k_edge2 and k_etile launch their own; so does the dense solver).
struct Pick { const void *fn; LdsLimit *lim; int threads; size_t lds; };

template <auto K> static Pick pick_of(int threads, size_t lds) {
    static LdsLimit lim;
    return Pick{reinterpret_cast<const void *>(K), &lim, threads, lds};
}

template <typename R, bool WIDE>
static Pick pick_tile(const PlanDev &pd, bool so, bool fused, bool prof) {
    constexpr int kThreads = WIDE ? 1024 : 512;
    const size_t lds = tile_lds_bytes_r(pd, so, sizeof(R), kThreads / 64);
    if (so && fused) return pick_of<&k_tile<true, false, WIDE, true, R>>(kThreads, lds);
    if (so) return pick_of<&k_tile<true, false, WIDE, false, R>>(kThreads, lds);
    if (prof) return pick_of<&k_tile<false, true, WIDE, false, R>>(kThreads, lds);
    return pick_of<&k_tile<false, false, WIDE, false, R>>(kThreads, lds);
}

// fused: the structure-only k_tile that also does the step's update; prof: the cycle-counting variant (BT_DEBUG_MODE 32 for
// k_tile, 16 for the solver)
static Pick pick(const PlanDev &pd, int K, bool so, bool fused, bool prof) {
    const Route &r = pd.route;
    if (K == 1) {
        if (r.kernel != Route::kTile) return Pick{};
        if (r.prec == 8) return pick_tile<double, false>(pd, so, fused, prof);
        return r.wide ? pick_tile<float, true>(pd, so, fused, prof) : pick_tile<float, false>(pd, so, fused, prof);
    }
    if (K == 4) {
        if (so) return pick_of<&k_update<true>>(kUpdThreads, 0);
        if (r.kernel == Route::kEtile) return Pick{};
        const size_t geo = (size_t)pd.max_tile_pairs * kUpdGeo;
        if (r.prec == 8) return pick_of<&k_update<false, kUpdThreads, double>>(kUpdThreads, (geo + kUpdThreads) * sizeof(double));
        if (r.wide) return pick_of<&k_update<false, 1024>>(1024, (geo + 1024) * sizeof(float));
        return pick_of<&k_update<false>>(kUpdThreads, (geo + kUpdThreads) * sizeof(float));
    }
    switch (r.solver) {
    case Route::kSolvePipe:
        return prof ? pick_of<&k_solve_pipe<true>>(kSolveThreads, solve_pipe_lds_bytes(pd)) : pick_of<&k_solve_pipe<false>>(kSolveThreads, solve_pipe_lds_bytes(pd));
    case Route::kSolveFused: {
        const size_t lds = solve_fused_lds_bytes(pd, kSolveThreads);
        return prof ? pick_of<&k_solve_fused<true>>(kSolveThreads, lds) : pick_of<&k_solve_fused<false>>(kSolveThreads, lds);
    }
    case Route::kSolveLds: {
        const size_t lds = solve_lds_bytes(pd, sizeof(double));
        return prof ? pick_of<&k_solve_lds<double, true>>(kSolveThreads, lds) : pick_of<&k_solve_lds<double, false>>(kSolveThreads, lds);
    }
    case Route::kSolveLds32: {
        const size_t lds = solve_lds_bytes(pd, sizeof(float));
        return prof ? pick_of<&k_solve_lds<float, true>>(kSolveThreads, lds) : pick_of<&k_solve_lds<float, false>>(kSolveThreads, lds);
    }
    case Route::kSolveGlobal: return pick_of<&k_solve_global>(1024, 0);
    default: return Pick{};
    }
}

// ev: the kernel's (start, stop) event pair, or nullptr; args: exactly the kernel's parameter types
template <typename... Args>
static void launch_pick(const Pick &p, unsigned grid, hipStream_t st, const hipEvent_t *ev, Args... args) {
    void *argv[] = {&args...};
    if (ev) (void)hipExtLaunchKernel(p.fn, dim3(grid), dim3(p.threads), argv, p.lds, st, ev[0], ev[1], 0);
    else (void)hipLaunchKernel(p.fn, dim3(grid), dim3(p.threads), argv, p.lds, st);      // (errors: hipGetLastError, as for <<< >>>)
}

int configure_kernels(PlanDev &pd) {
    pd.route = plan_route(pd);
    // the LDS limits of everything the route can launch, raised here at upload (never first inside a captured step); the
    // launchers of the other kernel families raise their own
    for (int K : {1, 3, 4})
        for (int v = 0; v < 8; ++v) {
            const Pick p = pick(pd, K, v & 1, v & 2, v & 4);
            if (!p.fn) continue;
            if (p.lds > kLdsBudget) return BT_EUNSUPPORTED;
            if (!p.lim->ensure(p.fn, p.lds, pd.dev_id)) return BT_EHIP;
        }
    return BT_OK;
}

// ev == nullptr: plain launches.  ev != nullptr: hipExtLaunchKernel with a (start, stop) event pair per kernel — ev[2*k],
// ev[2*k+1], k = 0 prep, 1 tile, 2 pair_finalize, 3 solve, 4 update, 5 the depth walk of the wave-per-tile plans — so bench.py
// can read each kernel's own duration on the stream it ran on.
int launch_reduce(const PlanDev &pd, const StepArgs &a, bool so, hipStream_t st, hipEvent_t *ev, unsigned *ran,
                  int fuse_so_poses, bool *fused) {
    const Route &r = pd.route;
    // a structure-only step in one launch: tile workgroups, then the rest of the patch buffer and the poses (k_tile, k_etile)
    const bool fuse = so && fuse_so_poses >= 0 && fused && pd.nlz == 0 && (r.kernel == Route::kTile || r.kernel == Route::kEtile);
    const int total = pd.p_tot + (fuse_so_poses > 0 ? pd.n_buf : 0);
    if (fused) *fused = fuse && pd.T > 0;
    if (ran && pd.T > 0) *ran |= 1u << 1;
    int rc = BT_OK;
    if (r.kernel == Route::kEdge || r.kernel == Route::kStream)
        rc = (r.kernel == Route::kEdge ? launch_edge : launch_stream)(pd, a, so ? 1 : 0, st, ev ? ev[2] : nullptr, ev ? ev[3] : nullptr);
    else if (r.kernel == Route::kEtile)
        // unfused structure-only step (multi-GPU phases, the timed path): the tile blocks only — they leave (Q, w') for the
        // k_update<true> that follows
        rc = launch_etile(pd, a, so ? 1 : 0, fuse ? fuse_so_poses : 0, fuse ? (total + 511) / 512 : 0, 0, st, ev ? ev[2] : nullptr, ev ? ev[3] : nullptr);
    else if (pd.T > 0) {
        const Pick p = pick(pd, 1, so, fuse, (a.dbg & 32) != 0);
        const int nbr = fuse ? (total + p.threads - 1) / p.threads : 0;
        launch_pick(p, pd.T + nbr, st, ev ? ev + 2 : nullptr, pd, a, fuse ? fuse_so_poses : 0);
    }
    if (rc != BT_OK) return rc;
    // the tracks that sit in no tile (more than 64 free cameras): their edges, their Schur terms (ba_loose.hip)
    rc = launch_loose_reduce(pd, a, so, st);
    if (rc != BT_OK) return rc;
    if (!so && pd.P > 0) {
        const int pb = (pd.P + 3) / 4, nt16 = pd.max_rows16 >> 4;
        const int sp_blocks = (r.kernel == Route::kEtile && pd.sp_ok) ? pd.sg_n * (nt16 * (nt16 + 1) / 2 + 1) : 0;
        if (ran) *ran |= 1u << 2;
        if (ev) hipExtLaunchKernelGGL(k_pair_finalize, dim3(pb + sp_blocks), dim3(256), 0, st, ev[4], ev[5], 0, pd, a, pb);
        else hipLaunchKernelGGL(k_pair_finalize, dim3(pb + sp_blocks), dim3(256), 0, st, pd, a, pb);
    }
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

int launch_pack(const PlanDev &pd, const StepArgs &a, bool unpack, hipStream_t st) {
    const int total = pd.nnzb * 36 + pd.D;
    if (total <= 0) return BT_OK;
    if (unpack) hipLaunchKernelGGL(k_pack_system<true>, dim3((total + 255) / 256), dim3(256), 0, st, pd, a);
    else        hipLaunchKernelGGL(k_pack_system<false>, dim3((total + 255) / 256), dim3(256), 0, st, pd, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

int launch_solve_update(const PlanDev &pd, const StepArgs &a, bool so, bool copy_poses, hipStream_t st, hipEvent_t *ev, unsigned *ran) {
    const Route &r = pd.route;
    if (!so) {
        if (ran) *ran |= 1u << 3;
        if (r.solver == Route::kSolveDense) {
            const int rc = launch_solve_dense(pd, a, st, ev ? ev[6] : nullptr, ev ? ev[7] : nullptr);
            if (rc != BT_OK) return rc;
        } else {
            const Pick p = pick(pd, 3, false, false, (a.dbg & 16) != 0);
            const bool f32 = r.solver == Route::kSolveLds32 || r.solver == Route::kSolveGlobal;
            const int passes = f32 ? 1 + kRefineSteps : 1;             // float32 factor: iterative refinement
            for (int pass = 0; pass < passes; ++pass) {
                if (pass >= 1) hipLaunchKernelGGL(k_refine_residual, dim3((pd.D + 3) / 4), dim3(256), 0, st, pd, a, pass > 1 ? 1 : 0);
                launch_pick(p, 1, st, pass == 0 && ev ? ev + 6 : nullptr, pd, a);          // (the event pair of kernel 3 times the first pass)
                if (pass >= 1 && pass == passes - 1) hipLaunchKernelGGL(k_refine_add, dim3(1), dim3(1024), 0, st, pd, a);
            }
        }
    }
    const int do_poses = so ? (copy_poses ? 1 : 0) : 1;
    const int total = pd.p_tot + (do_poses ? pd.n_buf : 0);
    const size_t nz = (size_t)pd.D * pd.D + pd.D;
    if (!so && (r.kernel == Route::kEdge || r.kernel == Route::kStream)) {
        // the tracks' depths by the wave-per-tile walk (event pair 5), then the rest in k_update
        if (ran) *ran |= 1u << 5;
        const int rc = (r.kernel == Route::kEdge ? launch_edge : launch_stream)(pd, a, 2, st, ev ? ev[10] : nullptr, ev ? ev[11] : nullptr);
        if (rc != BT_OK) return rc;
    }
    if (ran) *ran |= 1u << 4;
    if (!so && r.kernel == Route::kEtile) {
        const int nbe = (total + 511) / 512, zbe = (int)((nz + 4 * 512 - 1) / (4 * 512));
        const int rc = launch_etile(pd, a, 2, do_poses, nbe, zbe, st, ev ? ev[8] : nullptr, ev ? ev[9] : nullptr);
        if (rc != BT_OK) return rc;
    } else {
        // k_update: the k_tile route's tile blocks, the rest of the patch buffer and the poses, then the clearing of [S | y]
        const Pick p = pick(pd, 4, so, false, false);
        const int tb = !so && r.kernel == Route::kTile ? pd.T : 0;
        const int nb = (total + p.threads - 1) / p.threads, zb = so ? 0 : (int)((nz + 4 * p.threads - 1) / (4 * p.threads));
        launch_pick(p, tb + nb + zb, st, ev ? ev + 8 : nullptr, pd, a, do_poses, tb, tb + nb);
    }
    if (!so) { const int rc = launch_loose_update(pd, a, st); if (rc != BT_OK) return rc; }
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

}  // namespace bt
