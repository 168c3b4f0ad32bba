// ba_kernels.hpp — argument block, kernel picks and launchers shared by the kernel files of the BA step (ba_tile.hip,
// ba_pair.hip, ba_solve.hip, ba_xchg.hip and the later families), its sequence (ba_step.cpp) and ba_api.cpp.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_ext.h>

#include "ba_plan.hpp"
#include "dev_cache.hpp"

namespace bt {

// bt_ba_args plus the workspace regions, passed by value to every kernel.
struct StepArgs {
    const float *poses, *patches, *mono, *intr, *targets, *weights;
    int tstride, mstride;         // floats between consecutive edges' targets / patches' depth priors
    float *poses_out, *patches_out;
    float b0, b1, b2, b3, lmbda, ep, alpha;
    const float *lmbda_trk;       // per-track lmbda (ba.py:299-300) or nullptr
    int loss;
    double *S, *y, *pairacc;      // S, y, pairacc are contiguous (cleared together)
    double *priv;                 // private copies of y and the per-pair sums (ba_plan.hpp: kPrivY, kPrivP) or nullptr
    double *packed;               // the non-zero blocks of [S | y] in factor order (multi-GPU exchange buffer)
    float2 *qw;
    float *lfac, *linv, *zvec, *dx, *dx0;
    unsigned long long *dxg;      // [D] granules {float dx, uint32 tag}: dX as the solver of a fused solve + update launch publishes it (ba_solve_update.hpp)
    float *pairgeo;               // [pairs][kPairGeomFloats]: relative pose of every camera pair, left by k_tile for k_pair_finalize
    int *status;
    double *spart;                // [tiles][ntl * 256 + max_rows16]: per-tile Schur products of k_etile when the plan's sp_ok (else unused)
    double *esave;                // [tiles][max_rows16][1 << et_lgts]: the tiles' E (rows of the tile's cameras x its tracks), k_etile -> k_etile_upd
    int prec;                     // 1: the per-edge maths, E, pairgeo and qw are float64 (k_tile path, the default there); 0: float32
    int dbg;                      // env BT_DEBUG_MODE, 0 in production: 16 / 32 launch the cycle-counting variants of the solver / k_tile
};

// A kernel instantiation of a route with its workgroup, its dynamic LDS and the LDS limit kept for it.  fn == nullptr: the
// route launches none of that family (k_stream, k_edge2 and k_etile launch their own; so does the dense solver).
struct Pick { const void *fn; LdsLimit *lim; int threads; size_t lds; };

template <auto K> Pick pick_of(int threads, size_t lds) {
    static LdsLimit lim;              // one per kernel instantiation
    return Pick{reinterpret_cast<const void *>(K), &lim, threads, lds};
}

// ev: the kernel's (start, stop) event pair, or nullptr; args: exactly the kernel's parameter types
template <typename... Args>
void launch_pick(const Pick &p, unsigned grid, hipStream_t st, const hipEvent_t *ev, Args... args) {
    void *argv[] = {&args...};
    if (ev) (void)hipExtLaunchKernel(p.fn, dim3(grid), dim3(p.threads), argv, p.lds, st, ev[0], ev[1], 0);
    else (void)hipLaunchKernel(p.fn, dim3(grid), dim3(p.threads), argv, p.lds, st);      // (errors: hipGetLastError, as for <<< >>>)
}

// The picks of a route, per family.  fused: the structure-only k_tile that also does the step's update; prof: BT_DEBUG_MODE 32 / 16
Pick pick_tile(const PlanDev &pd, bool so, bool fused, bool prof);       // ba_tile.hip
Pick pick_update(const PlanDev &pd, bool so);                            // ba_tile.hip
Pick pick_solver(const PlanDev &pd, bool prof);                          // ba_solve.hip
Pick pick_solve_update(const PlanDev &pd);                               // ba_solve_update.hpp (fn == nullptr: the route launches solver and update apart)

// LDS of k_tile with per-edge numbers of rsz bytes and of the LDS-resident solvers: what plan_route weighs against kLdsBudget
size_t tile_lds_bytes_r(const PlanDev &pd, bool so, size_t rsz, size_t kTileWaves);
size_t solve_lds_bytes(const PlanDev &pd, size_t elem);
size_t solve_fused_lds_bytes(const PlanDev &pd, int nthreads);
size_t solve_pipe_lds_bytes(const PlanDev &pd);
// LDS of an update workgroup of the fused solve + update launch with `wgs` update workgroups, per-edge numbers of rsz bytes
size_t solve_update_lds_bytes(const PlanDev &pd, int wgs, size_t rsz);
// update workgroups of that launch (CU count - 1, capped by the work and by BT_FORCE updwg=N) and the tiles each of them holds
int solve_update_workgroups(const PlanDev &pd);
inline int solve_update_tiles_per_wg(const PlanDev &pd, int wgs) { return wgs > 0 ? (pd.T + wgs - 1) / wgs : 0; }
// 12 waves: enough helper threads for one round of update rows on banded systems, and a 170-register budget per thread so
// that a whole 6x6 operand block can be in flight from LDS
constexpr int kSolveThreads = 768;

// decides the plan's route (pd.route: which Jacobian kernel, per-edge precision and solver its steps launch) and raises the
// dynamic-LDS limit of every k_tile / k_update / solver instantiation that route can launch (ba_step.cpp)
int configure_kernels(PlanDev &pd);
// wave-per-tile streaming kernels (ba_stream.hip) for graphs of many tiles; mode 0 = pose+structure, 1 = structure-only,
// 2 = depth back-substitution
int launch_stream(const PlanDev &pd, const StepArgs &a, int mode, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
// the same for slot-uniform graphs in the edge-major layout (ba_edge2u.hip)
int launch_edge(const PlanDev &pd, const StepArgs &a, int mode, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
// its pose+structure reduce with two edges per lane (ba_edge2.hip)
int launch_edge2(const PlanDev &pd, const StepArgs &a, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
// the pair-major tile kernel (ba_etile.hip): mode 0 = pose+structure reduce, 1 = the whole structure-only step, 2 = a
// pose+structure step's last kernel
int launch_etile(const PlanDev &pd, const StepArgs &a, int mode, int do_poses, int extra_blocks, int zero_blocks, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
// ev != nullptr: a (start, stop) event pair per kernel; *ran gets bit k set for every kernel k that was launched
// fuse_so_poses >= 0 (and `fused` given): a structure-only step on the k_tile path also does the step's update in the same
// launch (fuse_so_poses = 1: copy the poses too) and sets *fused; the caller then skips launch_solve_update
int launch_reduce(const PlanDev &pd, const StepArgs &a, bool so, hipStream_t st, hipEvent_t *ev = nullptr, unsigned *ran = nullptr,
                  int fuse_so_poses = -1, bool *fused = nullptr);
// B and v from the per-pair sums, behind every Jacobian kernel of a pose+structure step (ba_pair.hip); ev0, ev1: event pair or nullptr
int launch_pair_finalize(const PlanDev &pd, const StepArgs &a, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
// the route's block-sparse solver with the refinement passes of a float32 factor (ba_solve.hip); ev: event pair or nullptr
int launch_solve(const PlanDev &pd, const StepArgs &a, hipStream_t st, const hipEvent_t *ev);
// solver and the step's last kernel in ONE launch (routes with Route::fuse_update; ba_solve_update.hpp); ev: the solver's event pair or nullptr
int launch_solve_update_fused(const PlanDev &pd, const StepArgs &a, hipStream_t st, const hipEvent_t *ev);
// dense [S | y] <-> its non-zero blocks in factor order (bt_ba_pack / bt_ba_unpack; ba_xchg.hip)
int launch_pack(const PlanDev &pd, const StepArgs &a, bool unpack, hipStream_t st);
// one-shot peer-write exchange of the packed [S | y] (ba_xchg.hip: k_xchg_push / k_xchg_pull)
constexpr int kMaxRanks = 16;
size_t xchg_bytes(const PlanDev &pd, int world);
int launch_xchg_push(const PlanDev &pd, const StepArgs &a, void *const *bufs, int world, int rank, long long epoch, hipStream_t st);
int launch_xchg_pull(const PlanDev &pd, const StepArgs &a, void *own, int world, long long epoch, hipStream_t st);
// after_reduce: the caller has launched launch_reduce in the same call, so k_pair_finalize has cleared the tags of the dX granules
// and the route may fuse solver and update; this half on its own (bt_ba_solve_update: the multi-GPU phases, tests that solve
// one reduced system several times) launches the two kernels apart, as it always has
int launch_solve_update(const PlanDev &pd, const StepArgs &a, bool so, bool copy_poses, hipStream_t st, hipEvent_t *ev = nullptr, unsigned *ran = nullptr,
                        bool after_reduce = false);
// tracks seen by more than 64 free cameras sit in no tile (ba_loose.hip): their part of the reduce phase / of the last kernel
int launch_loose_reduce(const PlanDev &pd, const StepArgs &a, bool so, hipStream_t st);
int launch_loose_update(const PlanDev &pd, const StepArgs &a, hipStream_t st);
// the dense solver of plans with more than 255 free poses (ba_dense.hip)
int launch_solve_dense(const PlanDev &pd, const StepArgs &a, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);

}  // namespace bt
