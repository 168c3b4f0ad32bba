// ba_plan.hpp — structure of one BA edge list, shared by the host planner
// (ba_plan.cpp), the kernels (ba_tile.hip and the other ba_*.hip) and the C ABI (ba_api.cpp, plan_shift.cpp).
#pragma once
#include <array>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/batrack_ba.h"

namespace bt {

constexpr int kLanes = 64;          // tracks per wave tile (one lane = one track)
constexpr int kTileCamSoft = 16;    // close a tile when its camera union would exceed this
constexpr int kTileCamHard = 64;    // a track that sees more free cameras than this sits in no tile: a LOOSE track (ba_loose.hip)
constexpr int kTileCamF64 = 32;     // ... and so does one that sees more than THIS, where a plan has only a few of them (kFewHubs): a tile of 32
constexpr int kFewHubs = 64;        //     cameras keeps its E in LDS as double, one of 33 .. 64 would turn the whole plan's per-edge maths to float32
constexpr int kMaxFree = 255;       // free poses the block-sparse solvers take (8-bit pose numbers in their tables)
constexpr int kMaxFreeWide = 2048;  // ... and the dense solver of larger systems (ba_dense.hip: the right-hand side lives in LDS)
constexpr int kPairAccStride = 32;  // doubles per camera pair (27 used: 21 Bjj + 6 gj)
// Private copies of y and of the per-pair sums for k_edge2 (ba_edge2.hip): thousands of waves end with atomics on the SAME few
// cache lines (y is 6n doubles in all; a pair's 27 sums are hit by every wave of its source frame) and atomics on one line are
// served one after the other — at 8.4M edges they were 35 of the kernel's 170 us.  A wave adds to copy (its index mod the count);
// k_pair_finalize adds the copies up and clears them.
constexpr int kPrivY = 16, kPrivP = 4;
// behind them: one arrival counter per SIMD of the chip (k_edge2: which of a SIMD's two waves am I — see "wave priority" there)
constexpr int kPrivArrive = 8192;   // ints: xcc (3 bits) | se (3) | sh (1) | cu (4) | simd (2)
constexpr int kPairGeomFloats = 20; // R(9) t(3) Ki(4) Kj(4)
constexpr int kLdsRowStride = 66;   // floats per local E row (bank-conflict-free)
constexpr int kMaxLevelCols = 4;    // columns of the reduced system factored concurrently (one critical wave each)
// LDS a solver workgroup may ask for (160 KB a CU), and what the block-sparse factor with its tables takes there at `elem` bytes
// per number: the planner sends systems whose factor does not fit as double to the dense solver (ba_plan_solver.cpp: `wide`).
constexpr size_t kLdsBudget = 160 * 1024 - 512;
inline size_t solve_lds_bytes_raw(size_t nnzb, size_t D, size_t nupd, size_t n, size_t nlev, size_t ndp, size_t elem) {
    size_t b = (nnzb * 36 + 2 * D) * elem;                                 // Lw, z, zt
    b = (b + 15) / 16 * 16;
    b += nupd * 3 * sizeof(unsigned short);                                // update triples
    b = (b + 15) / 16 * 16;
    // row_idx, col_ptr, upd_ptr, upd_next, dp_ptr, lvl_ptr, lvl_cols, dp
    b += (nnzb + 4 * (n + 1) + nlev + 1 + n + ndp) * sizeof(int);
    b = (b + 15) / 16 * 16 + nlev * kMaxLevelCols * 8 * sizeof(int);       // lvl_meta
    return b + 64;
}
constexpr int kSpGroupMax = 32;     // tiles per group of k_pair_finalize's positional sums of the tiles' Schur products
constexpr int kMaxTilePairs = 192;  // distinct camera pairs per tile whose geometry is kept in LDS

#ifdef __HIPCC__
#define BT_HD __host__ __device__
#else
#define BT_HD
#endif
// doubles of the private region (WsLayout::priv): the copies of y, of the per-pair sums, the arrival counters
BT_HD inline size_t priv_copy_doubles(size_t D, size_t pairs) { return (size_t)kPrivY * D + (size_t)kPrivP * pairs * kPairAccStride; }
BT_HD inline size_t priv_doubles(size_t D, size_t pairs) { return priv_copy_doubles(D, pairs) + kPrivArrive / 2; }
// doubles per tile of StepArgs::spart (plans with sp_ok): the tile's Schur product (ntl lower 16x16 tiles of 256), E Q w'
// (max_rows16) and its per-pair sums (max_tile_pairs x 32: 27 used)
BT_HD inline size_t sp_tile_doubles(int max_rows16, int max_tile_pairs) {
    const size_t nt = (size_t)max_rows16 / 16;
    return nt * (nt + 1) / 2 * 256 + (size_t)max_rows16 + (size_t)(max_tile_pairs > 0 ? max_tile_pairs : 1) * 32;
}

// LDS bytes of k_etile's pose+structure instantiation (ba_etile.hip) for a plan whose largest tile has max_rows16 rows of E
// and max_tile_pairs camera pairs, with per-edge numbers of rsz bytes: the planner lays a plan out for that kernel only if
// this fits (kEtileLdsBudget)
constexpr size_t kEtileLdsBudget = 160 * 1024 - 512;
BT_HD inline size_t etile_full_lds_bytes(int max_rows16, int max_tile_pairs, size_t rsz) {
    const size_t mtp = (size_t)(max_tile_pairs > 0 ? max_tile_pairs : 1), rows = (size_t)max_rows16;
    size_t smax = 1;
    while (smax < mtp) smax <<= 1;
    return (size_t)4 * 26 * smax * sizeof(double) + (rows * kLdsRowStride + 128 + mtp * kPairGeomFloats) * rsz + rows * sizeof(int) + 64;
}

// The kernels a plan's BA step launches: decided once per plan from its PlanDev scalars and BT_FORCE (ba_step.cpp:
// plan_route, called by configure_kernels) and read by the launchers only.
struct Route {
    enum : int { kTile = 0, kStream = 1, kEdge = 2, kEtile = 3 };          // kernel: the bt_plan_jacobian_kernel codes
    // solver: 0 .. 3 are the "solver_mode" readback (factor in LDS as double, in LDS as float, in the global workspace as
    // float, dense as double: wide plans); kSolveFused and kSolvePipe are variants of kSolveLds (k_solve_fused, k_solve_pipe)
    enum : int { kSolveLds = 0, kSolveLds32 = 1, kSolveGlobal = 2, kSolveDense = 3, kSolveFused = 4, kSolvePipe = 5 };
    int kernel;
    int prec;                     // bytes of the per-edge maths (bt_plan_edge_precision): 8 float64, 6 mixed (k_stream, k_edge2), 4 float32
    int wide;                     // kTile with float32 maths only: k_tile / k_update run 16 waves per tile instead of 8
    int solver;
    int fuse_update;              // pose+structure steps run the solver and the step's last kernel in one launch (ba_solve_update.hpp)
    int upd_wgs;                  // ... with this many update workgroups behind the solver's
};

// Device-side view: raw pointers into one device allocation + sizes.
struct PlanDev {
    int E, n_buf, p_tot, fixedp, n_all, n, D, m, P, T, slots, erows, nnzb, nupd, max_rows16;
    const int32_t *kx;
    const uint32_t *act_bits;                                // bit p: patch p has a track; [ceil(p_tot / 32)]
    const int32_t *act_rank;                                 // tracks before the word's first patch: track(p) = act_rank[p>>5] + popc(bits below p)
    const int32_t *pair_i, *pair_j;
    const int32_t *tile_trk0, *tile_ntrk, *tile_ncam, *tile_cam0, *tile_slot0, *tile_nslot, *tile_erow0;
    const int32_t *tile_cams;
    const int32_t *slot_edge, *slot_pair;
    const uint16_t *slot_lab;
    const int32_t *tile_pair0, *tile_npair, *tile_pairs;     // distinct camera pairs of a tile (global pair ids)
    const uint16_t *tile_cut8, *tile_cut16;                  // per tile: slot ranges of k_tile's 8 / 16 waves [9] / [17] (ba_plan.cpp)
    const int32_t *tile_ij, *tile_kx;                        // per tile: cameras of its pairs [max_tile_pairs], patch of its tracks [64]
    const int32_t *tile_flags;                               // bit 0: same cameras as the previous tile, bit 1: same pair list
    const uint8_t *slot_lp;                                  // local pair index of a (slot, lane) within its tile
    int max_tile_pairs, max_tile_slots, max_cams;
    long long e_all;                                         // length of the caller's edge list (slot_edge indexes it)
    const uint16_t *slot_code;                               // (slot, lane): local target camera | local pair << 8
    const uint8_t *tile_la;                                  // (tile, lane): local source camera of the lane's track (0xff: fixed)
    const int32_t *tile_rec;                                 // 8 ints per tile (ba_plan.cpp)
    const int32_t *it_edge;                                  // edge-major layout (ba_plan.cpp): [iterations][64]
    const uint32_t *tile_sinfo;                              // [tiles][64]
    const int32_t *pm_edge, *pm_rec;                         // pair-major layout (ba_plan.cpp): [rounds][64], [tiles][4]
    const uint8_t *pm_lb, *pm_la;                            // [tiles][64]: target camera of local pair s / source camera of track l
    const int32_t *pp_ptr, *pp_idx;                          // sp_ok: the (tile << 6 | local pair) entries of every camera pair, CSR over the pairs
    const int32_t *sg_ptr; int sg_n;                         // sp_ok: first tile of every group of consecutive same-camera tiles (sg_n + 1 entries)
    int et_lgts;                                             // sp_ok: log2 of the track stride of StepArgs::esave (>= the largest tile's tracks)
    int sp_ok;                                               // k_etile leaves per-tile Schur products and pair sums (StepArgs::spart) instead of atomics
    int pm_ok;                                               // the pair-major tables exist (every tile has at most 64 camera pairs)
    // LOOSE tracks (ba_plan.cpp): tracks seen by more than kTileCamHard free cameras sit in no tile; their edges are walked by
    // k_loose_reduce / k_loose_update (ba_loose.hip), a workgroup per track, the track's E in LDS over ALL free cameras
    const int32_t *lz_trk, *lz_ptr, *lz_edge, *lz_pair;      // track of loose track l; its edges [lz_ptr[l], lz_ptr[l + 1]): edge id, camera pair
    int nlz;
    int dev_id;                                              // the device the plan's tables live on (the launchers' per-device caches: no hipGetDevice per launch)
    int wide;                                                // more than kMaxFree free poses, or a factor too large for LDS as double: the dense solver (ba_dense.hip); perm is the identity, the packed form is the lower triangle by blocks
    int trk_off;                                             // sharded plan: distinct tracks of the full edge list in front of this rank's first
    int em_self;                                             // some edge has ii == jj (its source-camera E lands on a target row)
    int em_ok, em_its, em_lgs;                               // every tile slot-uniform; total iterations; log2 S if the same for all tiles, else -1
    int st_ok;                                               // the compact tables of k_stream exist (the plan was laid out for the wave-per-tile kernels)
    int st_min, em_min;                                      // stream_min_tiles() / edge_min_tiles() when the plan was built: the launch-time choice is the plan's own
    const int32_t *col_ptr, *row_idx, *upd_ptr, *upd, *blk_col, *upd_next;
    // elimination order and level schedule of the reduced solver
    int nlev, ndp;
    const int32_t *perm, *blk_src, *lvl_ptr, *lvl_cols, *col_lvl, *dp_ptr, *dp;
    // fused schedule (k_solve_fused): pending updates per destination block, lazy triples per column
    const int32_t *fz_pend_ptr, *fz_pend, *fz_lazy_ptr, *fz_lazy, *fz_yurg, *fz_meta, *fz_pmeta, *bs_sync, *fz_rowinfo, *fz_pfirst, *fz_psecond;
    int fz_npend, fz_nlazy, fz_ok;      // fz_ok: no level has more than two columns
    int fzp_ok;                         // and every column's panel fits one wave (k_solve_pipe)
    const int32_t *lvl_meta;   // [nlev][kMaxLevelCols][8]: col, diag pos, #sub-blocks, first rest triple, #rest triples, dp first, #dp, 0  (col = -1: unused)
    Route route;               // set by configure_kernels (host side only: no kernel reads it)
};

// Bytes of the status block at WsLayout::status: int 0 the solver status, 1 the exchange time-out, 2 the fused update's hand-off
// time-out (BT_SOLVE_HANDOFF_TIMEOUT, cleared by k_pair_finalize every step), 4.. profiling counters, 200 / 201
// the dense solver's flags, 210 the refinement's flag (ba_solve.hip, ba_dense.hip).  Cleared by bt_ba_workspace_init.
constexpr size_t kStatusBytes = 1024;
constexpr int kStatusHandoff = 2;

// Byte offsets of the regions inside the caller's workspace.
struct WsLayout {
    size_t sys, pairacc, zero_bytes;   // [sys, sys+zero_bytes): the accumulators; zero after bt_ba_workspace_init and after every completed
                                       // step (the kernels that consume them clear them; the reduce does not)
    size_t packed, pairgeo, qw, lfac, linv, zvec, dx, dx0, dxg, status, spart, esave, total;
    size_t priv;                       // inside the cleared region: [kPrivY][D] then [kPrivP][pairs][kPairAccStride] doubles; 0 = none
};

// The tables a plan uploads, in their order in the device buffer (ba_api.cpp: upload_plan): element type, name, and 1 for the
// tables of the block-sparse reduced solver (a wide plan has none: ba_plan_solver.cpp, go_wide).  Each name is a vector of bt_plan, a
// pointer of PlanDev and a name bt_plan_array answers to.
#define BT_PLAN_TABLES(X)                                                                                                      \
    X(int32_t, kx, 0) X(uint32_t, act_bits, 0) X(int32_t, act_rank, 0) X(int32_t, pair_i, 0) X(int32_t, pair_j, 0)              \
    X(int32_t, tile_trk0, 0) X(int32_t, tile_ntrk, 0) X(int32_t, tile_ncam, 0) X(int32_t, tile_cam0, 0)                         \
    X(int32_t, tile_slot0, 0) X(int32_t, tile_nslot, 0) X(int32_t, tile_erow0, 0) X(int32_t, tile_cams, 0)                       \
    X(int32_t, slot_edge, 0) X(int32_t, slot_pair, 0) X(uint16_t, slot_lab, 0)                                                  \
    X(int32_t, col_ptr, 1) X(int32_t, row_idx, 1) X(int32_t, upd_ptr, 1) X(int32_t, upd, 1) X(int32_t, blk_col, 1)              \
    X(int32_t, upd_next, 1) X(int32_t, lvl_meta, 1) X(int32_t, tile_flags, 0)                                                   \
    X(int32_t, tile_pair0, 0) X(int32_t, tile_npair, 0) X(int32_t, tile_pairs, 0) X(uint8_t, slot_lp, 0)                         \
    X(int32_t, perm, 1) X(int32_t, blk_src, 1) X(int32_t, lvl_ptr, 1) X(int32_t, lvl_cols, 1) X(int32_t, col_lvl, 1)            \
    X(int32_t, dp_ptr, 1) X(int32_t, dp, 1)                                                                                     \
    X(int32_t, fz_pend_ptr, 1) X(int32_t, fz_pend, 1) X(int32_t, fz_lazy_ptr, 1) X(int32_t, fz_lazy, 1) X(int32_t, fz_yurg, 1)   \
    X(int32_t, fz_meta, 1) X(int32_t, fz_pmeta, 1) X(int32_t, bs_sync, 1) X(int32_t, fz_rowinfo, 1) X(int32_t, fz_pfirst, 1)     \
    X(int32_t, fz_psecond, 1) X(int32_t, tile_ij, 0) X(int32_t, tile_kx, 0) X(uint16_t, tile_cut8, 0) X(uint16_t, tile_cut16, 0) \
    X(uint16_t, slot_code, 0) X(uint8_t, tile_la, 0) X(int32_t, tile_rec, 0) X(int32_t, it_edge, 0) X(uint32_t, tile_sinfo, 0)   \
    X(int32_t, pm_edge, 0) X(int32_t, pm_rec, 0) X(uint8_t, pm_lb, 0) X(uint8_t, pm_la, 0)                                      \
    X(int32_t, pp_ptr, 0) X(int32_t, pp_idx, 0) X(int32_t, sg_ptr, 0)                                                           \
    X(int32_t, lz_trk, 0) X(int32_t, lz_ptr, 0) X(int32_t, lz_edge, 0) X(int32_t, lz_pair, 0)

namespace tab {                       // table ids, in list order: bt_plan::off[tab::kx] ...
#define BT_TAB_ID(T, name, solver) name,
enum : int { BT_PLAN_TABLES(BT_TAB_ID) kCount };
#undef BT_TAB_ID
}  // namespace tab
constexpr int kNumTables = tab::kCount;

// Where a shifted clone stands with the proof that its list is the one it was made for (plan_shift.cpp).  Host side only.
struct SpecState {
    enum State : int {
        kNone,       // no speculation, or one that bt_plan_spec_confirm has settled
        kUnbound,    // made AHEAD of its list (bt_plan_preshift): no step before bt_plan_spec_bind
        kPolled,     // bound: no event — the verdict is complete when flag[2] holds `epoch` (bt_plan_spec_bind)
        kEvent       // the verdict lies behind `event` (bt_plan_create_shifted_spec)
    };
    State state = kNone;
    int *flag = nullptr;          // the verdict's pinned ints: [0] list differs, [1] index out of range, [2] the epoch of a polled one
    void *event = nullptr;        // kEvent: a hipEvent_t
    int epoch = 0;                // kPolled: > 0
    void *stream = nullptr;       // kPolled: the stream the comparison was launched on — what a poll that runs out of patience waits for
    bool unsettled() const { return state != kNone; }      // neither a shift source nor a confirmed plan
};

}  // namespace bt

// All of a plan but its vectors: what bt_plan::recycle resets in one assignment.  The scalars the kernels read live in `dev` only.
struct bt_plan_scalars {
    bt_plan_info info{};
    std::array<size_t, bt::kNumTables> off{};   // byte offsets of the tables inside the device buffer (ba_api.cpp: upload_plan)
    std::array<size_t, bt::kNumTables> len{};   // their element counts there, the tables the device writes included
    size_t dev_bytes = 0;          // bytes of the device buffer in use
    size_t pk_off = 0;             // packed edge list (kk << 32 | ii << 16 | jj, 8 bytes per edge) inside the device buffer, 0 = not kept
    int64_t trk_win_lo = 0;
    // plans whose pm_edge is written on the device (plan_device.hip): the table's rounds, and what the kernels need of the host's analysis
    int dev_pm = 0;
    int dev_slots = 0;                                        // likewise the [slots][64] arrays and the wave cuts of a 64-track layout
    int dev_wpt = 0;                                          // ... and with them the tables of the wave-per-tile kernels (slot_code, tile_la, it_edge, tile_sinfo)
    int64_t dev_f_lo = 0, dev_nw = 0;
    int64_t dev_q0 = 0;                                       // sharded: position of the rank's first edge in the device's sorted list
    long long pm_rounds = 0;
    bt::WsLayout ws{};
    void *dev_base = nullptr;   // one device allocation holding every table (from the pool in ba_api.cpp)
    // the stream the plan's kernels were last launched on: bt_plan_destroy records an event there, and the next plan that
    // reuses the device buffer makes its table upload wait for it (the tables must not change under queued kernels)
    mutable void *last_stream = nullptr;
    mutable bool launched = false;
    size_t dev_cap = 0;
    int64_t k_hi = -1;                                        // largest patch index the plan's tables hold (plan_shift.cpp: shift_fits checks k_hi + dk < p_tot)
    bt::SpecState spec{};                                     // a speculative clone's state (bt_plan_spec_confirm settles it)
    int is_clone = 0;                                         // made by clone_shifted (plan_shift.cpp): the host vectors are empty, bt_plan_array reads every table from the buffer
    bt::PlanDev dev{};            // the planner's scalars; upload_plan adds the table pointers
};

struct bt_plan : bt_plan_scalars {
#define BT_TAB_VEC(T, name, solver) std::vector<T> name;
    BT_PLAN_TABLES(BT_TAB_VEC)
#undef BT_TAB_VEC
    std::vector<int32_t> trk_loc;                                  // host only
    std::vector<int32_t> trk_win;                                  // track of patch trk_win_lo + i (-1: none): the window of patches the edges name
    mutable std::vector<int32_t> trk_of_patch;                     // the same over the whole patch buffer, expanded on request (bt_plan_array: tests)
    std::vector<char> stage;     // upload staging (kept with the object: ba_api.cpp)
    std::vector<int32_t> dev_off;                             // [m + 1]: first position of every track's edges in the grouped order
    std::vector<int32_t> dev_pbase;                           // aligned slot layout (ba_plan.cpp): first slot of every (tile, local pair), as tile_pairs; empty: a track's s-th edge is its slot s
    mutable std::vector<int32_t> dev_readback;                // bt_plan_array of a table the device wrote, and of the named figures
    std::vector<int32_t> dev_pair_of;                         // [nw * nw]: pair index of (i - f_lo, j - f_lo) or -1
    // hipEvent_t behind a clone's copies on the plan stream (ba_api.cpp: mark_launch), else null.  Atomic: two host threads may
    // launch the same fresh clone; whoever finds the event complete CLAIMS it (exchange) before handing it back to the pool —
    // handed back twice, two later clones would share one event.
    mutable std::atomic<void *> ready{nullptr};

    // Back to the state of a new object, but with the vectors' capacity kept: destroyed plans are recycled
    // by bt_plan_create (ba_api.cpp), so that a plan per frame costs no heap traffic.
    void recycle() {
        static_cast<bt_plan_scalars &>(*this) = bt_plan_scalars{};
        ready = nullptr;
#define BT_TAB_CLEAR(T, name, solver) name.clear();
        BT_PLAN_TABLES(BT_TAB_CLEAR)
#undef BT_TAB_CLEAR
        for (auto *v : {&trk_loc, &trk_win, &trk_of_patch, &dev_off, &dev_pbase, &dev_readback, &dev_pair_of}) v->clear();
        stage.clear();
    }
};

namespace bt {
// BT_FORCE — the ONE environment switch of the kernel / solver / planner choices (tests and measurement; production leaves it
// unset).  Comma-separated tokens, parsed once per process:
//   kernel=k_tile | k_stream | k_edge2 | k_etile   the Jacobian kernel every plan whose layout admits it takes
//   solver=fused | lds | lds32 | global            the reduced solver (default: k_solve_pipe where the plan allows it)
//   order=natural                                  no twisted elimination order
//   prec=f32                                       float32 per-edge maths on the k_tile path (round 2's numerics)
//   wide=0 | wide=1                                k_tile's 8 / 16 waves per tile
//   plan=host                                      no device-side planner
//   wpt=0                                          no wave-per-tile kernels (= bt_config_wave_per_tile_kernels(0))
//   upd=split                                      solver and k_update as two launches where the route would fuse them (A/B, tests)
//   updwg=N                                        at most N update workgroups in the fused launch, so that a small graph puts
//                                                  several tiles on one workgroup (test hook only)
//   wptwaves=N                                     at most N waves in the launches of k_edge2, k_edge2u and k_stream, so that a small
//                                                  graph puts several tiles on one wave (test hook only; nothing else of a launch changes)
struct Force {
    int kernel = -1;        // -1 the plan's own choice, 0 k_tile, 1 k_stream, 2 k_edge2, 3 k_etile
    int solver = -1;        // -1 default, 0 k_solve_fused (barrier per level), 1 k_solve_lds<double>, 2 k_solve_lds<float>, 3 k_solve_global
    int natural_order = 0, f32_edges = 0, tile_wide = -1, host_plan = 0, wpt_off = 0;
    int upd_split = 0, upd_wgs = 0;     // upd=split; updwg=N (0: no cap)
    int wpt_waves = 0;                  // wptwaves=N (0: no cap)
    int cap_waves(int max_waves) const { return wpt_waves > 0 && wpt_waves < max_waves ? wpt_waves : max_waves; }
};
const Force &force();
// BT_PLAN_PROF: time per planner phase on stderr (measurement)
bool plan_prof();
// tick("name"): the time since the tick before.  The planner's lines carry the label of the phase that comes next ("plan phase
// before"), the C ABI's (PhaseTimer tick{"plan api"}) that of the work just done.
struct PhaseTimer {
    const char *prefix = "plan phase before";
    bool on = plan_prof();
    std::chrono::steady_clock::time_point prev = std::chrono::steady_clock::now();
    void operator()(const char *name) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "%s %s: %.3f ms\n", prefix, name, std::chrono::duration<double, std::milli>(now - prev).count());
        prev = now;
    }
};
// Tile counts from which the wave-per-tile kernels take a graph (k_edge2, k_stream; the environment overrides are for
// measurement and tests).  The planner lays out their tables only for plans that will use them.
int edge_min_tiles();
int stream_min_tiles();
// the wave-per-tile kernels for graphs of >= 2048 tiles, on by default (bt_config_wave_per_tile_kernels); returns the previous setting
int config_wave_per_tile_kernels(int enable);
// Pure host analysis (no HIP).  Returns BT_OK or an error code.
// `packed` (optional): the edges as 8-byte words kk << 32 | ii << 16 | jj, already range-checked (ii / jj / kk are then not read)
// `dstats` (optional; plan_device.hip): the per-track figures of the edge list as a kernel gathered them — the analysis then
// reads NO edge: it lays out tracks, pairs, tiles and the reduced system from the tracks' (source frame, target mask), and
// leaves the one edge-sized table of a window plan (pm_edge) and the tiles' round counts to the device
// (bt_plan::dev_pm).  Returns BT_NEED_EDGES where that does not apply (the caller then runs the analysis on the edges).
struct PatchStat { int32_t cnt, src, src_min, pad; unsigned long long mask, mask2; };      // bit b of (mask | mask2 << 64): an edge into frame src - 64 + b
// the target frames a track observes MORE THAN ONCE (same bit numbering as PatchStat's masks): gathered for lists large enough
// for the wave-per-tile kernels, whose aligned slot layout needs to know where a track's extra edges can be
struct RepStat { unsigned long long rmask, rmask2; };
struct DevPlanStats {
    const PatchStat *tab;          // the patches tab_lo .. tab_lo + tab_n - 1: all the list names (kmin .. kmax), or — a rank's plan of a
    int64_t tab_lo, tab_n;         // sharded solve — only those of its own range: the rank's host share is then ~ its share of the tracks
    int64_t kmin, kmax, n_all, f_lo;
    int any_self;
    int rep_known;                 // the repeated targets were looked for (rtab null then means: there are none)
    const RepStat *rtab;           // as tab, or null
    // a rank's plan: what it needs to know of the OTHER ranks' tracks, reduced on the device from the full table
    int sliced;                    // tab holds the own range only
    int64_t trk_before, edges_before;      // distinct tracks / edges of the patches in front of the range
    const uint32_t *pattern;       // [n][pattern_words] bits: free cameras u >= v that some track of the list couples (null: n = 0 or a wide plan)
    int pattern_words;
};
enum { BT_NEED_EDGES = 2 };
// fn(frame) for every target frame of a track's masks, ascending (bit b of mask | mask2 << 64: frame base + b)
template <class F> inline void for_targets(uint64_t mask, uint64_t mask2, int32_t base, F &&fn) {
    for (uint64_t mk = mask; mk; mk &= mk - 1) fn((int32_t)(base + __builtin_ctzll(mk)));
    for (uint64_t mk = mask2; mk; mk &= mk - 1) fn((int32_t)(base + 64 + __builtin_ctzll(mk)));
}
// The reduced camera system of a plan whose tiles, pairs and loose tracks are laid out (ba_plan_solver.cpp; called by
// build_plan_host): the block-sparse solvers' tables, or `wide`.  `pk` / `E`: the packed edge list, read by a sharded plan
// without `dstats` only.
int plan_reduced_system(bt_plan *plan, bool sharded, const DevPlanStats *dstats, const uint64_t *pk, int64_t E, PhaseTimer &tick);
int build_plan_host(const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E,
                    int64_t n_buf, int64_t p_tot, int64_t fixedp, int64_t n_all_min,
                    int64_t own_lo, int64_t own_hi, bt_plan *plan, const uint64_t *packed = nullptr, bool keep_slots = false,
                    const DevPlanStats *dstats = nullptr);
// the same packing on the device (plan_pack.hip): `out` E words and `bad` one int (set to 1 on an index out of range), device memory
int launch_shift_match(const uint64_t *nw, const uint64_t *ow, int64_t E, int *out, void *stream);
// pack the list into `out` and set host_flags[0] unless word[e] == ow[e] + delta for every edge, host_flags[1] on an index out of
// range (bt_plan_create_shifted_spec; host_flags: device-visible pinned memory, cleared by the caller)
int launch_pack_match_expect(const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E, int64_t n_buf, int64_t p_tot,
                             const uint64_t *ow, uint64_t delta, uint64_t *out, int *host_flags, void *stream);
// the list against `ow` word for word; host_flags (pinned): [0] differs, [1] index out of range, [2] = epoch once every workgroup is through
int launch_match_done(const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E, int64_t n_buf, int64_t p_tot,
                      const uint64_t *ow, int *host_flags, unsigned *ticket, int epoch, void *stream);
int launch_words_add(const uint64_t *ow, uint64_t delta, uint64_t *out, int64_t E, void *stream);
int launch_plan_shift(int32_t *kx, int m, int32_t *tile_kx, int nkx, int32_t *tile_ij, int nij, int32_t *pair_i, int32_t *pair_j, int P,
                      const uint32_t *old_bits, uint32_t *new_bits, int32_t *new_rank, int nwords, int df, int dk, void *stream);
int launch_pack_edges(const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E, int64_t n_buf, int64_t p_tot,
                      uint64_t *out, int *bad, void *stream);
int pack_edges_host(const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E, int64_t n_buf, int64_t p_tot, uint64_t *out);
// the passes over the edges on the device (plan_device.hip; bt_plan_create)
int plan_device_stats(const uint64_t *d_words, int64_t E, int64_t p_tot, int64_t fixedp, int64_t own_lo, int64_t own_hi, void *stream, DevPlanStats *st, int64_t *tracks);
int plan_device_rounds(const bt_plan *pl, int64_t E, void *stream, int64_t *rounds);
int plan_device_fill(const bt_plan *pl, int64_t E, int32_t *d_rec, int32_t *d_pm_edge, int64_t rounds, void *stream);
int plan_device_slots_stage(const bt_plan *pl, void *stream);
// the tables of the wave-per-tile kernels, written by the same passes (device pointers into the plan's buffer; tile_rec is the
// host's upload, the passes add the straddle flag; it_edge / tile_sinfo null: the layout of k_edge2 does not apply)
struct DevWptOut { uint16_t *slot_code; uint8_t *tile_la; int32_t *tile_rec; int32_t *it_edge; uint32_t *tile_sinfo; int64_t its; };
int plan_device_slots_fill(const bt_plan *pl, int64_t E, int32_t *d_slot_edge, int32_t *d_slot_pair, uint16_t *d_slot_lab, uint8_t *d_slot_lp,
                           uint16_t *d_cut8, uint16_t *d_cut16, void *stream, const DevWptOut *wpt = nullptr);
// after the stream of plan_device_slots_fill has been waited for: 1 = some tile is not slot-uniform (no k_edge2 for this plan)
int plan_device_em_verdict();
// Copies the arrays to the device and fills plan->dev (ba_api.cpp).  `d_packed` (optional): the packed edge list on the device,
// kept behind the tables where the plan may become a shift source.
int upload_plan(bt_plan *plan, const uint64_t *d_packed = nullptr);
}  // namespace bt
