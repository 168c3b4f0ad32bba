// ba_solve_update.hpp — k_solve_update: the reduced solver and the step's last kernel (k_update, ba_tile.hip) in ONE launch,
// for the k_tile routes whose solver is one of the LDS-resident double ones (plan_route / configure_kernels, ba_step.cpp).
// A header of ba_solve.hip alone (included at its end, never compiled by itself): workgroup 0 runs that file's solver body as
// a device function, and device functions do not link across objects.
//
// While the one solver workgroup runs, the rest of the GPU is idle, and everything k_update does but its last multiply-adds
// is independent of dX.  So the launch is 1 + W workgroups of the solver's size (768 threads, one per CU):
//   workgroup 0       the route's solver, unchanged; where it writes dX it also publishes it as tagged granules
//                     (StepArgs::dxg, ba_update.hpp).  It is dispatched first and never waits for anybody.
//   workgroups 1..W   update workgroups, the roles dealt by grid stride:
//     patch role      copy + clamp of the patches that carry no track (update_rest): needs no dX, runs at once
//     tile role       waves 0..7, with k_update<false, 512>'s slot partition, for the tiles wg, wg + W, ...: BEFORE dX the
//                     slot tables, targets, weights, patch, (Q, w'), the pair geometry into LDS and edge_eval; what the
//                     last lines of k_update's slot loop read — a0, a2..a5, b1..b5, W0 jz0, W1 jz1 and the edge's local
//                     pair (-1: no edge) — stays in LDS per (slot, lane).  AFTER dX: per edge delta of its camera pair from
//                     dX, the slot products summed through part[] in k_update's order, clamp, store.
//     pose role       waves 8..11: Exp(dX) G
//     zero role       waves 8..11: [S | y] cleared once dX has arrived (the solvers admitted here have taken S into
//                     LDS by then, retries included: they publish behind their attempt loop)
// The hand-off.  Before dX, waves 8..11 list the granules their workgroup needs (the free cameras of its tiles, its poses);
// then every lane of them polls ONE granule of the list until it carries the tag, and leaves the value in LDS (dxc).  One
// trip to memory brings everything: a single polling lane in front of it (the first form measured here) put a second,
// dependent trip behind the first, 0.7 us each on the idle chip (profiles/r22_solve_update.txt).  A workgroup polls 6 to 8
// cache lines every ~0.2 us.
// The rehearsal.  What follows dX runs TWICE, same code: once before the wait on made-up dX with its global stores switched
// off, then for real.  The first pass costs nothing (the workgroup would be waiting) and was meant to leave the second's
// instructions in the instruction cache.  It has NOT been measured on its own: the wall-clock stamps of r22 show the first
// (cold) pass of a phase no slower than the second, so its gain is unproven; the A/B of r22 is of the kernel with it.
// The arithmetic is k_update's, the same functions (pair_delta, edge_term: ba_edge.hpp; new_disp: ba_update.hpp): fused and split
// steps give the same bits.
// Every wait is bounded: a lane that has polled for kSuPollTicks (~100 ms) writes BT_SOLVE_HANDOFF_TIMEOUT to the status
// block and takes dX = 0 for its granule; the workgroup writes its outputs and returns.
#pragma once
#include "ba_edge.hpp"
#include "ba_update.hpp"

namespace bt {

constexpr int kSuTileThreads = 512;            // threads of the tile role: k_update<false, 512>'s eight waves
constexpr int kSuSaved = 12;                   // numbers kept per (slot, lane)
constexpr long long kSuPollTicks = 10000000;   // poll budget in ticks of the 100 MHz wall clock: 100 ms

// LDS of an update workgroup per tile it holds: reals (geo[pairs][kUpdGeo], saved[slots][kSuSaved][64], the track's
// (x, y, disparity, Q, w')[64], part[8][64]) and ints (local pair per (slot, lane), patch[64], the free cameras of every pair, 4 scalars)
BT_HD inline size_t su_tile_reals(size_t mtp, size_t msl) { return mtp * kUpdGeo + msl * kSuSaved * 64 + 5 * 64 + (kSuTileThreads / 64) * 64; }
BT_HD inline size_t su_tile_ints(size_t mtp, size_t msl) { return msl * 64 + 64 + 2 * mtp + 4; }
// ... and per workgroup: dxc[D] floats, the list of the granules it needs (6 per camera of a tile and per pose it retracts)
BT_HD inline size_t su_need_ints(const PlanDev &pd, int wgs, int tiles) {
    return (size_t)tiles * 6 * (size_t)(pd.max_cams > 0 ? pd.max_cams : 1) + 6 * (size_t)((pd.n_buf + wgs - 1) / wgs) + 4;
}

size_t solve_update_lds_bytes(const PlanDev &pd, int wgs, size_t rsz) {
    const size_t mtp = pd.max_tile_pairs > 0 ? (size_t)pd.max_tile_pairs : 1, msl = (size_t)pd.max_tile_slots;
    const int tiles = solve_update_tiles_per_wg(pd, wgs);
    return (size_t)tiles * (su_tile_reals(mtp, msl) * rsz + su_tile_ints(mtp, msl) * sizeof(int)) +
           (4 + (size_t)pd.D + su_need_ints(pd, wgs, tiles)) * sizeof(int) + 16;
}

int solve_update_workgroups(const PlanDev &pd) {
    DevProps dp;
    if (!device_props(&dp, pd.dev_id)) return 0;
    const long long nz = (long long)pd.D * pd.D + pd.D;
    // work items: tiles, blocks of patches, poses, blocks of [S | y]
    const long long items = (long long)pd.T + (pd.p_tot + kSolveThreads - 1) / kSolveThreads + pd.n_buf + (nz + 1023) / 1024;
    long long w = items < dp.n_cu - 1 ? items : dp.n_cu - 1;
    if (force().upd_wgs > 0 && w > force().upd_wgs) w = force().upd_wgs;
    return w < 1 ? 1 : (int)w;
}

template <typename R>
__device__ __forceinline__ void su_update_workgroup(const PlanDev &pd, const StepArgs &a, unsigned char *smem, int wg, int W, int tpw) {
    typedef typename Vec2<R>::type R2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    constexpr int kWaves = kSuTileThreads / 64;
    const int mtp = pd.max_tile_pairs > 0 ? pd.max_tile_pairs : 1, msl = pd.max_tile_slots;
    const size_t tileR = su_tile_reals((size_t)mtp, (size_t)msl), tileI = su_tile_ints((size_t)mtp, (size_t)msl);
    R *baseR = reinterpret_cast<R *>(smem);
    int *baseI = reinterpret_cast<int *>(baseR + (size_t)tpw * tileR);
    int *sync = baseI + (size_t)tpw * tileI;                                  // [4]: waves of the tile role that have left their partial sums
    float *dxc = reinterpret_cast<float *>(sync + 4);                         // [D]: dX as this workgroup has received it
    int *need = reinterpret_cast<int *>(dxc + pd.D);                          // the granules it needs
    const int h = tid - kSuTileThreads, nh = (int)blockDim.x - kSuTileThreads;   // waves 8..: pollers, pose and zero role
    int nneed = 0;
    if (tid == 0) sync[0] = 0;

    // ---- patch role
    for (long long gid = (long long)wg * blockDim.x + tid; gid < pd.p_tot; gid += (long long)W * blockDim.x)
        update_rest<false, true>(pd, a, (int)gid, 0);

    // ---- tile role, before dX
#pragma unroll 1
    for (int k = 0; k < tpw; ++k) {
        const int tile = wg + k * W;
        if (tile >= pd.T) break;
        R *geo = baseR + (size_t)k * tileR, *sav = geo + (size_t)mtp * kUpdGeo, *trk = sav + (size_t)msl * kSuSaved * 64;
        int *lpv = baseI + (size_t)k * tileI, *pch = lpv + (size_t)msl * 64, *cam = pch + 64, *meta = cam + 2 * mtp;
        int patch = -1, slot0 = 0, s0 = 0, s1 = 0;
        R px = 0, py = 0, pdisp = 0;
        SlotStream<R> ss;
        if (tid < kSuTileThreads) {
            const int np = pd.tile_npair[tile], nslot = pd.tile_nslot[tile];
            patch = pd.tile_kx[(size_t)tile * kLanes + lane];
            slot0 = pd.tile_slot0[tile];
            wave_slots(nslot, wave, kWaves, s0, s1);
            if (tid == 0) { meta[0] = nslot; meta[1] = np; }
            if (s0 < s1) ss.start(pd, slot0 + s0, lane);
            for (int p = tid; p < np; p += kSuTileThreads) {
                const int gp = pd.tile_pairs[pd.tile_pair0[tile] + p];
                cam[2 * p] = pd.pair_i[gp] - pd.fixedp; cam[2 * p + 1] = pd.pair_j[gp] - pd.fixedp;
                // (workspace -> LDS, the values are not needed in registers here: a copy of its own, not load_pairgeo.  Through
                //  load_pairgeo the float64 instantiations issue the ten loads in front of the stores, the scalar-register spills
                //  around the solver's body move — some 300 instructions of k_solve_update<*, double> — and the C3 step measured
                //  0.3 us slower, profiles/r23_update_once.txt)
                const R2 *src = reinterpret_cast<const R2 *>(reinterpret_cast<const R *>(a.pairgeo) + (size_t)gp * kPairGeomFloats);
                R2 *o = reinterpret_cast<R2 *>(geo + (size_t)p * kUpdGeo);
#pragma unroll
                for (int c = 0; c < kPairGeomFloats / 2; ++c) o[c] = src[c];
                R2 zero; zero.x = (R)0; zero.y = (R)0;
                o[13] = zero;
            }
            if (patch >= 0) { px = a.patches[3*patch]; py = a.patches[3*patch + 1]; pdisp = a.patches[3*patch + 2]; }
            ss.fetch(a);
            if (wave == 0) {
                R2 qw; qw.x = (R)0; qw.y = (R)0;
                if (patch >= 0) qw = reinterpret_cast<const R2 *>(a.qw)[pd.tile_trk0[tile] + lane];
                trk[lane] = px; trk[64 + lane] = py; trk[128 + lane] = pdisp; trk[192 + lane] = qw.x; trk[256 + lane] = qw.y;
                pch[lane] = patch;
            }
        }
        else {                                                     // the granules of the tile's free cameras
            const int ncam = pd.tile_ncam[tile];
            const int *cams = pd.tile_cams + pd.tile_cam0[tile];
            for (int i = h; i < 6 * ncam; i += nh) need[nneed + i] = 6 * cams[i / 6] + i % 6;
        }
        nneed += 6 * pd.tile_ncam[tile];
        __syncthreads();
        if (tid < kSuTileThreads) {
#pragma unroll 1
            for (int s = s0; s < s1; ++s) {
                ss.advance(pd, a, slot0 + s + 1, s + 1 < s1, lane);
                const int e = ss.e, lp = ss.lp;
                R g[kPairGeomFloats];
                load16<kPairGeomFloats>(geo + (size_t)lp * kUpdGeo, g);
                EdgeQT<R> q;
                edge_eval<R>(g, px, py, pdisp, ss.tu, ss.tv, ss.w0, ss.w1, a, q);
                lpv[s * 64 + lane] = e < 0 ? -1 : lp;
                if (e < 0) continue;
                R *o = sav + (size_t)s * kSuSaved * 64 + lane;
                o[0] = q.a0; o[64] = q.a2; o[128] = q.a3; o[192] = q.a4; o[256] = q.a5;
                o[320] = q.b1; o[384] = q.b2; o[448] = q.b3; o[512] = q.b4; o[576] = q.b5;
                o[640] = q.W0 * q.jz0; o[704] = q.W1 * q.jz1;
            }
        }
    }

    // ... and of the poses this workgroup retracts: thread h of waves 8.. has pose wg + h W (-1: a fixed pose, no granule)
    const int npose = wg < pd.n_buf ? (pd.n_buf - wg + W - 1) / W : 0;
    for (int j = h; j >= 0 && j < npose; j += nh) {
        const long long p = wg + (long long)j * W;
        const bool fr = p >= pd.fixedp && p < pd.fixedp + pd.n;
        for (int c = 0; c < 6; ++c) need[nneed + 6 * j + c] = fr ? 6 * ((int)p - pd.fixedp) + c : -1;
    }
    nneed += 6 * npose;
    // ... and one granule in any case: a workgroup with no tile and no free pose still clears its share of [S | y], which it
    // may only do once the solver has published (it has S in LDS for good by then)
    if (h == 0) need[nneed] = 0;
    nneed += 1;

    const long long deadline = wall_clock64() + kSuPollTicks;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const bool real = pass == 1;
        if (!real) {
            for (int i = tid; i < pd.D; i += (int)blockDim.x) dxc[i] = 1e-3f;      // the rehearsal's dX (not 0: Exp takes its general branch)
        } else if (h >= 0) {
            // ---- the hand-off: one granule per lane, looked at until it carries this step's tag
            for (int i = h; i < nneed; i += nh) {
                const int k = need[i];
                if (k < 0) continue;
                float v;
                bool got = dx_peek(a, k, v);
                while (!got && wall_clock64() < deadline) { __builtin_amdgcn_s_sleep(8); got = dx_peek(a, k, v); }
                if (!got) { v = 0.0f; a.status[kStatusHandoff] = BT_SOLVE_HANDOFF_TIMEOUT; }
                dxc[k] = v;
            }
        }
        __syncthreads();
        if (h >= 0) {
            // ---- pose role: Exp(dX) * G (update_rest's pose branch), the pose's own thread both times
            for (long long p = wg + (long long)h * W; p < pd.n_buf; p += (long long)nh * W) {
                float xi[6] = {0, 0, 0, 0, 0, 0};
                if (p >= pd.fixedp && p < pd.fixedp + pd.n)
                    for (int c = 0; c < 6; ++c) xi[c] = dxc[6 * ((int)p - pd.fixedp) + c];
                float po[7];
                retract_pose(a.poses + 7*p, xi, po);
                if (real) for (int c = 0; c < 7; ++c) a.poses_out[7*p + c] = po[c];
            }
            // ---- zero role
            const size_t nz = (size_t)pd.D * pd.D + pd.D;
            if (real) for (size_t i = (size_t)wg * nh + h; i < nz; i += (size_t)W * nh) a.S[i] = 0.0;
        } else {
            // ---- tile role, after dX.  Behind the barrier above its eight waves meet only each other, through a counter in
            // LDS: the pose and zero roles of waves 8.. are off their path.  delta = dX_j - Ad(Gij) dX_i of the edge's camera
            // pair is formed by the edge's own thread (pair_delta, as in k_update, which forms it once per pair: same bits).
#pragma unroll 1
            for (int k = 0; k < tpw; ++k) {
                if (wg + k * W >= pd.T) break;
                const R *geo = baseR + (size_t)k * tileR, *sav = geo + (size_t)mtp * kUpdGeo;
                R *part = baseR + (size_t)k * tileR + (size_t)mtp * kUpdGeo + (size_t)msl * kSuSaved * 64 + 5 * 64;
                const int *lpv = baseI + (size_t)k * tileI, *cam = lpv + (size_t)msl * 64 + 64, *meta = cam + 2 * mtp;
                int s0, s1;
                wave_slots(meta[0], wave, kWaves, s0, s1);
                R acc = 0;
#pragma unroll 1
                for (int s = s0; s < s1; ++s) {
                    const int lp = lpv[s * 64 + lane];
                    if (lp < 0) continue;
                    const int ia = cam[2 * lp], ib = cam[2 * lp + 1];
                    R g[12], dl[6];                                            // the pair's R and t
                    load16<12>(geo + (size_t)lp * kUpdGeo, g);
                    pair_delta(g, dxc, ia, ib, dl);
                    const R *o = sav + (size_t)s * kSuSaved * 64 + lane;
                    EdgeQT<R> q;
                    q.a0 = o[0]; q.a2 = o[64]; q.a3 = o[128]; q.a4 = o[192]; q.a5 = o[256];
                    q.b1 = o[320]; q.b2 = o[384]; q.b3 = o[448]; q.b4 = o[512]; q.b5 = o[576];
                    acc += edge_term(q, o[640], o[704], dl);
                }
                part[wave * 64 + lane] = acc;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) __hip_atomic_fetch_add(sync, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            // the tracks' new disparities: wave k takes the workgroup's k-th tile, once all eight partial sums are there
            for (int k = wave; k < tpw; k += kWaves) {
                if (wg + k * W >= pd.T) break;
                wait_ge(sync, kWaves * (pass + 1));
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                const R *trk = baseR + (size_t)k * tileR + (size_t)mtp * kUpdGeo + (size_t)msl * kSuSaved * 64, *part = trk + 5 * 64;
                const int patch = (baseI + (size_t)k * tileI + (size_t)msl * 64)[lane];
                if (patch < 0) continue;
                R tot = 0;
#pragma unroll
                for (int w = 0; w < kWaves; ++w) tot += part[w * 64 + lane];
                const R px = trk[lane], py = trk[64 + lane], pdisp = trk[128 + lane];
                const float dd = new_disp<R>(pdisp, trk[192 + lane], trk[256 + lane], tot);
                if (real) { a.patches_out[3*patch] = (float)px; a.patches_out[3*patch + 1] = (float)py; a.patches_out[3*patch + 2] = dd; }
            }
        }
        if (!real) __syncthreads();          // (the pollers of the second pass write dxc)
    }
}

// SOLVER: Route::kSolvePipe, kSolveFused or kSolveLds (the double one); R: the precision of the per-edge maths (k_update's)
template <int SOLVER, typename R>
__global__ __launch_bounds__(kSolveThreads) void k_solve_update(PlanDev pd, StepArgs a, int tpw) {
    if (blockIdx.x == 0) {
        if constexpr (SOLVER == Route::kSolvePipe) solve_pipe_body<false, true>(pd, a);
        else if constexpr (SOLVER == Route::kSolveFused) solve_fused_body<false, true>(pd, a);
        else solve_lds_body<double, false, true>(pd, a);
        return;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    su_update_workgroup<R>(pd, a, smem, (int)blockIdx.x - 1, (int)gridDim.x - 1, tpw);
}

template <typename R>
static Pick pick_solve_update_of(int solver, size_t lds) {
    switch (solver) {
    case Route::kSolvePipe:  return pick_of<&k_solve_update<Route::kSolvePipe, R>>(kSolveThreads, lds);
    case Route::kSolveFused: return pick_of<&k_solve_update<Route::kSolveFused, R>>(kSolveThreads, lds);
    case Route::kSolveLds:   return pick_of<&k_solve_update<Route::kSolveLds, R>>(kSolveThreads, lds);
    default: return Pick{};
    }
}

// every workgroup of the launch carries the larger of the solver's LDS and an update workgroup's
Pick pick_solve_update(const PlanDev &pd) {
    const Route &r = pd.route;
    if (!r.fuse_update) return Pick{};
    const size_t rsz = r.prec == 8 ? sizeof(double) : sizeof(float);
    const size_t upd = solve_update_lds_bytes(pd, r.upd_wgs, rsz), sol = pick_solver(pd, false).lds;
    const size_t lds = upd > sol ? upd : sol;
    return r.prec == 8 ? pick_solve_update_of<double>(r.solver, lds) : pick_solve_update_of<float>(r.solver, lds);
}

int launch_solve_update_fused(const PlanDev &pd, const StepArgs &a, hipStream_t st, const hipEvent_t *ev) {
    const Pick p = pick_solve_update(pd);
    if (!p.fn) return BT_EUNSUPPORTED;
    launch_pick(p, 1u + (unsigned)pd.route.upd_wgs, st, ev, pd, a, solve_update_tiles_per_wg(pd, pd.route.upd_wgs));
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

}  // namespace bt
