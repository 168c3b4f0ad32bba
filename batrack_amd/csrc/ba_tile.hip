// ba_tile.hip — k_tile and k_update: the first and the last kernel of a BA step on the k_tile route (gfx950, wave64).
// One BA_rgbd_droid call (the reference's backend/ba.py:217-339) becomes four launches
//   k_tile           one workgroup of 8 (16) waves per tile of up to 64 tracks: relative pose of
//                    the tile's camera pairs (Gij is per PAIR, not per edge: projective_ops.py:61),
//                    per-edge reprojection, Jacobians, robust weights (projective_ops.py:54-100,
//                    ba.py:228-266), per-track C / w / E, per-pair J^T W J, and the tile's Schur
//                    product E Q E^T on the f64 MFMA (ba.py:284-323)
//   k_pair_finalize  B and v of ba.py:279-290 from the per-pair sums (ba_pair.hip)
//   k_solve_*        damped block-sparse Cholesky of the reduced camera system in LDS, forward and
//                    back substitution (ba.py:60-70,323-325; ba_solve.hip)
//   k_update         back-substitution of the depths, clamp of the whole buffer, pose retraction
//                    (ba.py:328-337, groups.py:153-156); leaves [S | y] clear for the next step
// plus k_pack_system for the multi-GPU exchange form (ba_xchg.hip); ba_step.cpp has the sequence (structure-only: k_tile<SO> + k_update<SO>).
// Algebra used throughout: Ji = -Jj * Ad(Gij), so with
// per-pair sums  Bjj = sum Jj^T W Jj,  gj = sum Jj^T W r  the blocks are
//   B[a,a] += Ad^T Bjj Ad   B[b,a] += -Bjj Ad   B[b,b] += Bjj
//   v[a]   += -Ad^T gj      v[b]   += gj        E[a,k] += -Ad^T Ej   E[b,k] += Ej
// and Ji is never formed per edge.
#include <hip/hip_runtime.h>

#include "ba_kernels.hpp"
#include "probe.hpp"
#include "ba_edge.hpp"
#include "ba_update.hpp"
#include "ba_wave.hpp"

namespace bt {

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
                    a.patches_out[3*patch] = (float)px; a.patches_out[3*patch + 1] = (float)py; a.patches_out[3*patch + 2] = new_disp<R>(pdisp, Q, wp, (R)0);
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

// ------------------------------------------------------------------ k_update
// One BA step's last kernel.  Block ranges (512 threads each):
//   [0, tile_blocks)         pose+structure steps only: one block per tile of tracks.  The depth update
//                            dZ_k = Q_k (w'_k - sum_c E[c,k]^T dX_c) (ba.py:328) is evaluated WITHOUT a stored E:
//                            E[c,k]^T dX_c summed over the cameras of a track is, edge by edge,
//                            Jz^T W (Jj dX_j + Ji dX_i) = Jz^T W Jj (dX_j - Ad(Gij) dX_i)  (Ji = -Jj Ad, projective_ops.py:96),
//                            so the block forms delta = dX_j - Ad dX_i (pair_delta, ba_edge.hpp) once per camera pair of the
//                            tile (from the pair geometry k_tile left in the workspace) and re-evaluates the edge Jacobians from
//                            targets / weights: 16 B per edge read again instead of 24 B per edge written and read back.
//   [.., + patch_blocks)     the whole patch buffer: copy of x, y and the clamp of ba.py:333; structure-only steps
//                            add dZ = Q w' (ba.py:316-317) here; pose+structure steps skip the patches that carry
//                            a track (the tile blocks write those).  Followed by one thread per buffer pose:
//                            Exp(dX) * G in double (groups.py:153-156).
//   [first_zero_block, ..)   [S | y] has been consumed by the solver: cleared for the next step's accumulation.
constexpr int kUpdThreads = 512;     // (kUpdGeo, the floats per pair in LDS: ba_update.hpp)

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
        const int slot0 = pd.tile_slot0[tile];
        int s0, s1;
        wave_slots(pd.tile_nslot[tile], wave, kWaves, s0, s1);
        SlotStream<R> ss;
        if (s0 < s1) ss.start(pd, slot0 + s0, lane);
        for (int p = tid; p < np; p += THREADS) {
            const int gp = pd.tile_pairs[pd.tile_pair0[tile] + p];
            R g[kPairGeomFloats], dl[6];
            load_pairgeo(a.pairgeo, gp, g);
            pair_delta(g, a.dx, pd.pair_i[gp] - pd.fixedp, pd.pair_j[gp] - pd.fixedp, dl);
            R *o = geo + (size_t)p * kUpdGeo;
#pragma unroll
            for (int c = 0; c < kPairGeomFloats; ++c) o[c] = g[c];
#pragma unroll
            for (int c = 0; c < 6; ++c) o[20 + c] = dl[c];
            o[26] = (R)0; o[27] = (R)0;
        }
        R px = 0, py = 0, pdisp = 0;
        if (patch >= 0) { px = a.patches[3*patch]; py = a.patches[3*patch + 1]; pdisp = a.patches[3*patch + 2]; }
        ss.fetch(a);
        __syncthreads();
        R acc = 0;
#pragma unroll 1
        for (int s = s0; s < s1; ++s) {
            ss.advance(pd, a, slot0 + s + 1, s + 1 < s1, lane);
            R g[kUpdGeo];
            load16<kUpdGeo>(geo + (size_t)ss.lp * kUpdGeo, g);
            EdgeQT<R> q;
            edge_eval<R>(g, px, py, pdisp, ss.tu, ss.tv, ss.w0, ss.w1, a, q);
            if (ss.e < 0) continue;
            acc += edge_term(q, q.W0 * q.jz0, q.W1 * q.jz1, g + 20);
        }
        part[wave * 64 + lane] = acc;
        __syncthreads();
        if (wave == 0 && patch >= 0) {
            R tot = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) tot += part[w * 64 + lane];
            const R2 qw = reinterpret_cast<const R2 *>(a.qw)[pd.tile_trk0[tile] + lane];
            a.patches_out[3*patch] = (float)px; a.patches_out[3*patch + 1] = (float)py; a.patches_out[3*patch + 2] = new_disp<R>(pdisp, qw.x, qw.y, tot);
        }
        return;
    }
    update_rest<SO, !SO>(pd, a, (int)(blockIdx.x - (SO ? 0 : tile_blocks)) * (int)blockDim.x + (int)threadIdx.x, do_poses);
}

// ------------------------------------------------------------------ the picks of the two families
// rsz: sizeof(R) of the k_tile instantiation
size_t tile_lds_bytes_r(const PlanDev &pd, bool so, size_t rsz, size_t kTileWaves) {
    const size_t rows = so ? 0 : (size_t)pd.max_rows16;
    const size_t mtp = pd.max_tile_pairs > 0 ? (size_t)pd.max_tile_pairs : 1;
    return (rows * kLdsRowStride + kTileWaves * 8 * 64 + 128 + mtp * kPairGeomFloats) * rsz + (kTileWaves * 64 + rows) * sizeof(int) + 64;
}

template <typename R, bool WIDE>
static Pick pick_tile_of(const PlanDev &pd, bool so, bool fused, bool prof) {
    constexpr int kThreads = WIDE ? 1024 : 512;
    const size_t lds = tile_lds_bytes_r(pd, so, sizeof(R), kThreads / 64);
    if (so && fused) return pick_of<&k_tile<true, false, WIDE, true, R>>(kThreads, lds);
    if (so) return pick_of<&k_tile<true, false, WIDE, false, R>>(kThreads, lds);
    if (prof) return pick_of<&k_tile<false, true, WIDE, false, R>>(kThreads, lds);
    return pick_of<&k_tile<false, false, WIDE, false, R>>(kThreads, lds);
}

Pick pick_tile(const PlanDev &pd, bool so, bool fused, bool prof) {
    const Route &r = pd.route;
    if (r.kernel != Route::kTile) return Pick{};
    if (r.prec == 8) return pick_tile_of<double, false>(pd, so, fused, prof);
    return r.wide ? pick_tile_of<float, true>(pd, so, fused, prof) : pick_tile_of<float, false>(pd, so, fused, prof);
}

Pick pick_update(const PlanDev &pd, bool so) {
    const Route &r = pd.route;
    if (so) return pick_of<&k_update<true>>(kUpdThreads, 0);
    if (r.kernel == Route::kEtile) return Pick{};
    const size_t geo = (size_t)pd.max_tile_pairs * kUpdGeo;
    if (r.prec == 8) return pick_of<&k_update<false, kUpdThreads, double>>(kUpdThreads, (geo + kUpdThreads) * sizeof(double));
    if (r.wide) return pick_of<&k_update<false, 1024>>(1024, (geo + 1024) * sizeof(float));
    return pick_of<&k_update<false>>(kUpdThreads, (geo + kUpdThreads) * sizeof(float));
}

}  // namespace bt
