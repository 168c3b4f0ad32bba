// ba_step.cpp — the sequence of a BA step: which kernels a plan's steps launch (plan_route), their LDS limits
// (configure_kernels) and the two halves of a step (launch_reduce, launch_solve_update).  No kernel lives here: the families
// are ba_tile.hip, ba_etile.hip, ba_stream.hip, ba_edge2.hip / ba_edge2u.hip, ba_loose.hip (Jacobians, update), ba_pair.hip,
// ba_solve.hip, ba_dense.hip (reduced system) and ba_xchg.hip (multi-GPU exchange).
#include <hip/hip_runtime_api.h>

#include "ba_kernels.hpp"

namespace bt {

// ------------------------------------------------------------------ the plan's route
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

// Solver and the step's last kernel in one launch (k_solve_update, ba_solve_update.hpp): the 8-wave k_tile routes whose solver
// is one of the double LDS ones, on plans with camera pairs (k_pair_finalize, which every such step launches, clears the
// granules' tags), where the tiles an update workgroup holds fit its LDS.  BT_FORCE upd=split: two launches, as every other route.
static void plan_fuse_update(PlanDev &pd) {
    Route &r = pd.route;
    r.fuse_update = 0; r.upd_wgs = 0;
    const bool solver_ok = r.solver == Route::kSolvePipe || r.solver == Route::kSolveFused || r.solver == Route::kSolveLds;
    if (force().upd_split || r.kernel != Route::kTile || r.wide || !solver_ok || pd.P <= 0 || pd.T <= 0 || pd.n <= 0) return;
    const int w = solve_update_workgroups(pd);
    if (w <= 0 || solve_update_lds_bytes(pd, w, r.prec == 8 ? sizeof(double) : sizeof(float)) > kLdsBudget) return;
    r.fuse_update = 1; r.upd_wgs = w;
}

int configure_kernels(PlanDev &pd) {
    pd.route = plan_route(pd);
    plan_fuse_update(pd);
    // the LDS limits of everything the route can launch, raised here at upload (never first inside a captured step); the
    // launchers of the other kernel families raise their own
    for (int v = 0; v < 8; ++v)
        for (const Pick &p : {pick_tile(pd, v & 1, v & 2, v & 4), pick_solver(pd, v & 4), pick_update(pd, v & 1), pick_solve_update(pd)}) {
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
        const Pick p = pick_tile(pd, so, fuse, (a.dbg & 32) != 0);
        const int nbr = fuse ? (total + p.threads - 1) / p.threads : 0;
        launch_pick(p, pd.T + nbr, st, ev ? ev + 2 : nullptr, pd, a, fuse ? fuse_so_poses : 0);
    }
    if (rc != BT_OK) return rc;
    // the tracks that sit in no tile (more than 64 free cameras): their edges, their Schur terms (ba_loose.hip)
    rc = launch_loose_reduce(pd, a, so, st);
    if (rc != BT_OK) return rc;
    if (!so && pd.P > 0) {
        if (ran) *ran |= 1u << 2;
        return launch_pair_finalize(pd, a, st, ev ? ev[4] : nullptr, ev ? ev[5] : nullptr);
    }
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

int launch_solve_update(const PlanDev &pd, const StepArgs &a, bool so, bool copy_poses, hipStream_t st, hipEvent_t *ev, unsigned *ran, bool after_reduce) {
    const Route &r = pd.route;
    if (!so && r.fuse_update && after_reduce && a.dbg == 0) {
        // one launch: the solver's workgroup and the update workgroups behind it (timed: under the solver's event pair; the
        // update's `ran` bit stays clear)
        if (ran) *ran |= 1u << 3;
        int rc = launch_solve_update_fused(pd, a, st, ev ? ev + 6 : nullptr);
        if (rc == BT_OK) rc = launch_loose_update(pd, a, st);
        if (rc != BT_OK) return rc;
        return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
    }
    if (!so) {
        if (ran) *ran |= 1u << 3;
        const int rc = r.solver == Route::kSolveDense ? launch_solve_dense(pd, a, st, ev ? ev[6] : nullptr, ev ? ev[7] : nullptr)
                                                      : launch_solve(pd, a, st, ev ? ev + 6 : nullptr);
        if (rc != BT_OK) return rc;
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
        const Pick p = pick_update(pd, so);
        const int tb = !so && r.kernel == Route::kTile ? pd.T : 0;
        const int nb = (total + p.threads - 1) / p.threads, zb = so ? 0 : (int)((nz + 4 * p.threads - 1) / (4 * p.threads));
        launch_pick(p, tb + nb + zb, st, ev ? ev + 8 : nullptr, pd, a, do_poses, tb, tb + nb);
    }
    if (!so) { const int rc = launch_loose_update(pd, a, st); if (rc != BT_OK) return rc; }
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

}  // namespace bt
