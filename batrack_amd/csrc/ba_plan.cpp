// ba_plan.cpp — host analysis of one BA edge list (no HIP calls in this file).
//
// What the reference recomputes inside every BA_rgbd_droid call
//   n = max(ii, jj) + 1                      /root/reference/main/backend/ba.py:219
//   kx, kk' = torch.unique(kk, sorted=True)  /root/reference/main/backend/ba.py:276
//   dense E [n, m, 6] scatter targets        /root/reference/main/backend/ba.py:284-285
// is done here once per edge list, and laid out for the tile kernel:
//   * tracks sorted by patch slot; a TILE is up to 64 consecutive tracks whose
//     union of free cameras stays small; lane l of the tile's wave owns track l;
//   * SLOT s of a tile holds the s-th edge of each of its tracks (edges of a track
//     ordered by camera pair, so tracks with the same observation pattern put
//     the same pair in the same slot and the per-pair reductions are wave-uniform);
//   * the distinct (ii, jj) camera pairs (their relative pose is per pair, not per edge);
//   * the block-sparsity of the reduced camera system and of its Cholesky factor (ba_plan_solver.cpp).
//
// build_plan_host runs the phases below in order.  The edge pass, the numbering of tracks and pairs and the grouping run once;
// everything from the tiling on is one LAYOUT attempt (lay_out), which a phase may ask to have repeated with one knob of
// `Layout` changed: 64-track tiles instead of 16, no aligned slots, hub tracks in tiles.
#include "ba_plan.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <unordered_map>

namespace bt {

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Tile counts from which a plan is laid out for the wave-per-tile kernels k_stream / k_edge2 (2048: profiles/r02_kernel_choice.txt).
// Those kernels evaluate an edge in MIXED precision since round 4 (reprojection and residual in float64, Jacobians and their
// products in float32: ba_edge.hpp edge_eval_mixed) and keep the update within north_star's 1e-5 of the reference's float64
// run (measured 1e-6 .. 5e-6 on the benchmark graphs; S and y 1e-7).  A caller who wants the reduced system itself to 1e-10
// at every size switches them off — bt_config_wave_per_tile_kernels(0) — and every plan then takes the float64-per-edge tile
// kernels (a third of the throughput from 2048 tiles on).  BT_FORCE (ba_plan.hpp) forces one kernel for every plan (tests,
// measurement).  A plan records what it was laid out for (st_ok,
// em_ok, st_min, em_min): the launch-time choice never depends on a later change of this setting.
const Force &force() {
    static const Force f = [] {
        Force r;
        const char *e = std::getenv("BT_FORCE");
        if (!e) return r;
        std::string s(e);
        size_t pos = 0;
        while (pos <= s.size()) {
            const size_t end = std::min(s.find(',', pos), s.size());
            const std::string tok = s.substr(pos, end - pos);
            pos = end + 1;
            if (tok == "kernel=k_tile") r.kernel = 0; else if (tok == "kernel=k_stream") r.kernel = 1;
            else if (tok == "kernel=k_edge2") r.kernel = 2; else if (tok == "kernel=k_etile") r.kernel = 3;
            else if (tok == "solver=fused") r.solver = 0; else if (tok == "solver=lds") r.solver = 1;
            else if (tok == "solver=lds32") r.solver = 2; else if (tok == "solver=global") r.solver = 3;
            else if (tok == "order=natural") r.natural_order = 1; else if (tok == "prec=f32") r.f32_edges = 1;
            else if (tok == "wide=0") r.tile_wide = 0; else if (tok == "wide=1") r.tile_wide = 1;
            else if (tok == "plan=host") r.host_plan = 1; else if (tok == "wpt=0") r.wpt_off = 1;
            else if (tok == "upd=split") r.upd_split = 1;
            else if (tok.rfind("updwg=", 0) == 0 && std::atoi(tok.c_str() + 6) > 0) r.upd_wgs = std::atoi(tok.c_str() + 6);
            else if (tok.rfind("wptwaves=", 0) == 0 && std::atoi(tok.c_str() + 9) >= 0) r.wpt_waves = std::atoi(tok.c_str() + 9);
            else if (!tok.empty()) std::fprintf(stderr, "batrack: unknown BT_FORCE token '%s'\n", tok.c_str());
        }
        return r;
    }();
    return f;
}
bool plan_prof() { static const bool p = std::getenv("BT_PLAN_PROF") != nullptr; return p; }

static std::atomic<int> g_wpt_kernels{-1};           // -1: not set by the caller -> BT_FORCE decides (default on)
static int wpt_env() { return force().wpt_off ? 0 : 1; }
int config_wave_per_tile_kernels(int enable) {
    const int prev = g_wpt_kernels.load();
    if (enable >= 0) g_wpt_kernels.store(enable ? 1 : 0);
    return prev < 0 ? wpt_env() : prev;
}
static int wpt_kernels_on() {
    const int v = g_wpt_kernels.load();
    return v >= 0 ? v : wpt_env();
}
constexpr int kNever = 1 << 30;
int edge_min_tiles() {
    const int k = force().kernel;
    return k == 2 ? 1 : k >= 0 ? kNever : (wpt_kernels_on() ? 2048 : kNever);
}
int stream_min_tiles() {
    const int k = force().kernel;
    return (k == 1 || k == 2) ? 1 : k >= 0 ? kNever : (wpt_kernels_on() ? 2048 : kNever);
}
// the pair-major layout (k_etile): 1 = for the plans it was measured on (few tiles, deep tracks), 0 = never, 2 = every plan
static int etile_mode() { const int k = force().kernel; return k == 3 ? 2 : k >= 0 ? 0 : 1; }

static void layout_workspace(bt_plan *pl) {
    const bt_plan_info &I = pl->info;
    const size_t D = (size_t)(6 * I.n);
    WsLayout w{};
    size_t off = 0;
    w.sys = off;      off += (D * D + D) * sizeof(double);
    off = align_up(off, 256);
    w.pairacc = off;  off += (size_t)I.pairs * kPairAccStride * sizeof(double);
    off = align_up(off, 256);
    w.priv = 0;
    if (I.tiles >= pl->dev.em_min) {   // (plans k_edge2 can take: by the tile count alone — whether the tiles are slot-uniform is, for
                                       //  a device-planned list, known only after the upload, and the layout must not depend on the planner)
        w.priv = off;
        off = align_up(off + priv_doubles(D, (size_t)I.pairs) * sizeof(double), 256);
    }
    w.zero_bytes = off - w.sys;
    w.packed = off;   off = align_up(off + ((size_t)I.nnz_blocks * 36 + D) * sizeof(double), 256);   // exchange form of [S | y]
    w.pairgeo = off;  off = align_up(off + (size_t)I.pairs * kPairGeomFloats * sizeof(double), 256);         // k_tile -> k_pair_finalize (float or double)
    w.qw = off;       off = align_up(off + (size_t)I.m * 2 * sizeof(double), 256);                           // (Q, w') per track (float2 or double2)
    // (a wide plan's dense factor: D x D doubles and the right-hand side behind it)
    w.lfac = off;     off = align_up(off + (pl->dev.wide ? (D * D + D) * sizeof(double) : (size_t)I.nnz_blocks * 36 * sizeof(float)), 256);
    w.linv = off;     off = align_up(off + (size_t)I.n * 36 * sizeof(float), 256);
    w.zvec = off;     off = align_up(off + D * sizeof(float), 256);
    w.dx = off;       off = align_up(off + D * sizeof(float) + 64, 256);
    w.dx0 = off;      off = align_up(off + D * sizeof(float) + 64, 256);     // first solution of a refined solve (float32-factor systems)
    w.status = off;   off = align_up(off + kStatusBytes, 256);
    w.dxg = off;      off = align_up(off + D * sizeof(unsigned long long), 256);   // dX as tagged granules (fused solve + update launch)
    w.spart = off;
    if (pl->dev.sp_ok) off = align_up(off + (size_t)I.tiles * sp_tile_doubles(pl->dev.max_rows16, pl->dev.max_tile_pairs) * sizeof(double), 256);
    w.esave = off;                                                 // k_etile -> k_etile_upd: the tiles' E, [tile][max_rows16][1 << et_lgts]
    if (pl->dev.sp_ok) off = align_up(off + (((size_t)I.tiles * pl->dev.max_rows16) << pl->dev.et_lgts) * sizeof(double), 256);
    w.total = off;
    pl->ws = w;
    pl->info.workspace_bytes = (int64_t)w.total;
}

// Edges as the planner reads them: one 8-byte word per edge, kk << 32 | ii << 16 | jj (n_buf <= 32768, p_tot < 2^31).
// For index tensors on the device the words are packed (and range-checked) by a kernel and copied back in one piece —
// a third of the bytes of the three int64 arrays (ba_api.cpp); host arrays are packed here.
int pack_edges_host(const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E, int64_t n_buf, int64_t p_tot, uint64_t *out) {
    for (int64_t e = 0; e < E; ++e) {
        if (ii[e] < 0 || jj[e] < 0 || ii[e] >= n_buf || jj[e] >= n_buf) return BT_EINVAL;
        if (kk[e] < 0 || kk[e] >= p_tot) return BT_EINVAL;
        out[e] = ((uint64_t)kk[e] << 32) | ((uint64_t)ii[e] << 16) | (uint64_t)jj[e];
    }
    return BT_OK;
}

namespace {

// Per patch, what ONE pass over the edges leaves (32 bytes a patch: the later passes stream a million of these): edges, source
// frame, and the set of target frames as 128 bits around the source frame — mask, mask2: target frames base + b and
// base + 64 + b, base = the source frame - 64, in the host's own pass as in the device's table.
struct PerPatch { int32_t cnt, src, base, last_j; uint64_t mask, mask2; };

// Edge- and patch-sized temporaries persist per thread: the caller builds one plan per frame, and fresh pages cost more than the
// passes over them.
struct PlanScratch {
    std::vector<uint64_t> pk;                            // the packed words of a host edge list
    std::unordered_map<int64_t, RepStat> rep_host;       // per patch the targets it observes more than once (host pass)
    std::vector<PerPatch> pp_tab;                        // indexed by patch; only [pp_lo, pp_hi] — [kmin, kmax] of the previous plan — is dirty
    int64_t pp_lo = 0, pp_hi = -1;
    std::vector<int32_t> off;                            // (a million tracks: no fresh pages per plan)
    std::vector<int32_t> ord, byj;
    std::vector<uint64_t> pks;
    std::vector<uint32_t> pm_code;
};
PlanScratch &scratch() { static thread_local PlanScratch s; return s; }

// What a layout attempt may not (or no longer) do.  Every knob moves once, in one direction.
struct Layout {
    bool small_tiles_allowed = true;     // 16-track tiles for k_etile
    bool aligned_allowed = true;         // slots per (pair, repeat) for k_edge2
    int cam_hard = kTileCamF64;          // a track of more free cameras than this is loose
};
// a phase's request to lay the plan out again with that knob changed (never leaves build_plan_host)
enum : int { kRelayoutLargeTiles = 1000, kRelayoutUnaligned, kRelayoutHubsInTiles };

struct PlanBuild {
    // the inputs
    int64_t E, n_buf, p_tot, fixedp, own_lo, own_hi;
    bool sharded;
    const uint64_t *pk;
    const DevPlanStats *dstats;
    bool keep_slots;
    bt_plan *pl;
    PhaseTimer tick;                                               // measurement only: time per phase on stderr
    // what the edge pass derives
    int64_t n_all, n = 0, kmin, kmax, f_lo, nw = 0, E_own = 0;    // [kmin, kmax]: patches the edges name (a window of the buffer);
    int32_t m = 0;                                                 // f_lo: first frame they name (the window's start, not the buffer's)
    bool sorted = true, masks_ok = true, mono_j = true;            // mono_j: within every track the target frames come in ascending order
    bool src_ok = true, any_self = false;
    int em_min_p = 0, st_min_p = 0;
    std::vector<int32_t> cj;                                       // edges per target frame (host pass)
    bt_plan_info info0{};                                          // pl->info as a layout attempt finds it
    // views of the per-thread scratch, and the pair table
    PerPatch *pp = nullptr;
    std::vector<int32_t> &off, &ord;                               // off: first position of a track's edges in the grouped order; ord: the edge there
    std::vector<uint64_t> &pks;                                    // ... and its packed word
    std::unordered_map<int64_t, RepStat> &rep_host;
    std::vector<int32_t> pair_of;                                  // [nw * nw]: pair of (i - f_lo, j - f_lo) or -1
    // one layout attempt
    Layout lay;
    int tcap = kLanes;
    bool aligned = false;
    std::vector<int32_t> loose;                                    // tracks seen by more than cam_hard free cameras
    std::vector<uint64_t> tile_tmask;                              // aligned: per tile the union of its tracks' target masks (2 words)
    int64_t slots = 0, erows = 0, pm_rounds_acc = 0;
    int max_cams = 0;
    bool dev_slots = false, want_slots = false, pm_direct = false, pm_fail = false, want_stream_tables = false, dev_wpt = false;

    explicit PlanBuild(PlanScratch &s) : off(s.off), ord(s.ord), pks(s.pks), rep_host(s.rep_host) {}
    int64_t KK(int64_t e) const { return (int64_t)(pk[e] >> 32); }
    int64_t II(int64_t e) const { return (int64_t)((pk[e] >> 16) & 0xffff); }
    int64_t JJ(int64_t e) const { return (int64_t)(pk[e] & 0xffff); }
    bool owned(int64_t e) const { return KK(e) >= own_lo && KK(e) < own_hi; }
    int64_t IQ(int64_t q) const { return (int64_t)((pks[(size_t)q] >> 16) & 0xffff); }      // frames of the q-th edge of the grouped order
    int64_t JQ(int64_t q) const { return (int64_t)(pks[(size_t)q] & 0xffff); }
    int32_t pair_ij(int64_t i, int64_t j) const { return pair_of[(size_t)((i - f_lo) * nw + (j - f_lo))]; }
    int32_t pair_q(int64_t q) const { return pair_ij(IQ(q), JQ(q)); }
    const int32_t *pair_row(int64_t src) const { return pair_of.data() + (size_t)(src - f_lo) * nw - f_lo; }      // row[target frame]
    int32_t trk_of(int64_t k) const { return pl->trk_win[(size_t)(k - kmin)]; }
    const PerPatch &track(int32_t k) const { return pp[pl->kx[(size_t)k]]; }
    bool same_targets(const PerPatch &t, int32_t src, int32_t base, uint64_t mask, uint64_t mask2) const {
        return t.src == src && t.base == base && t.mask == mask && t.mask2 == mask2;
    }
};

inline int ceil_log2(int x) { int lg = 0; while ((1 << lg) < x) ++lg; return lg; }
inline void clear_pair_major(bt_plan *pl) { pl->pm_edge.clear(); pl->pm_rec.clear(); pl->pm_lb.clear(); pl->pm_la.clear(); }
// position in pm_edge of (iteration l / G, round d, lane (l % G) * S + lp) of a tile whose rounds start at round0
inline size_t pm_index(int64_t round0, int32_t l, int32_t G, int32_t D, int32_t d, int lg, int32_t lp) {
    return ((size_t)round0 + (size_t)(l / G) * D + (size_t)d) * kLanes + (size_t)((l % G) << lg) + (size_t)lp;
}

// Iterations of an edge-major tile (64 / S tracks each): an EVEN number (the last one empty where the tile's tracks end in an
// odd one), so that the flat iteration stream of a wave pairs up (2J, 2J + 1) inside every tile — k_edge2 (ba_edge2.hip) takes
// two iterations per step, one edge of each per lane.  Also for S = 1, where one iteration is the whole tile: its second
// iteration is a row of -1 (k_edge2 reads rows 2J and 2J + 1 whatever S is; an odd count would hand it the next tile's row).
inline int32_t em_iterations(int32_t ntrk, int32_t G) {
    const int32_t nit = (ntrk + G - 1) / G;
    return (nit + 1) & ~1;
}

// ---- ONE pass over the edges: n_all (ba.py:219), the window of patches and frames they name, edges per track and per
// target frame, the camera pairs in use, and per track its source frame and the set of its target frames (a 64-bit mask
// around the first target seen: a track's observations span a window of frames, batrack.py:399-410)
// (The targets a track observes MORE THAN ONCE — the aligned slot layout's multiplicities — are kept aside, looked up only for
//  the tracks whose count exceeds their distinct targets: the device's table where it gathered them, a map filled by the host's
//  own pass)
void scan_edges(PlanBuild &b) {
    PerPatch *pp = b.pp;
    const uint64_t *pk = b.pk;
    const int64_t E = b.E, own_lo = b.own_lo, own_hi = b.own_hi;
    int64_t n_all = b.n_all, kmin = b.kmin, kmax = b.kmax, f_lo = b.f_lo, E_own = 0, k_prev = -1;
    bool sorted = true, masks_ok = true, mono_j = true, src_ok = true, any_self = false;
    int32_t *cj = b.cj.data();
    for (int64_t e = 0; e < E; ++e) {
        const int64_t k = (int64_t)(pk[e] >> 32), i = (int64_t)((pk[e] >> 16) & 0xffff), j = (int64_t)(pk[e] & 0xffff);
        any_self |= i == j;
        n_all = std::max(n_all, std::max(i, j) + 1);
        f_lo = std::min(f_lo, std::min(i, j));
        kmin = std::min(kmin, k); kmax = std::max(kmax, k);
        if (k < k_prev) sorted = false;
        k_prev = k;
        if (k < own_lo || k >= own_hi) continue;
        ++E_own;
        ++cj[(size_t)j + 1];
        PerPatch &t = pp[k];
        // (128 bits around the SOURCE frame, as the device's table has them: a list is laid out the same way wherever its indices live)
        if (t.cnt++ == 0) { t.src = (int32_t)i; t.base = (int32_t)i - 64; t.mask = 0; t.mask2 = 0; }
        else { if (t.src != (int32_t)i) src_ok = false; if ((int32_t)j < t.last_j) mono_j = false; }
        t.last_j = (int32_t)j;          // one source frame per track: the caller builds ii = ix[kk] (batrack.py:199)
        const int64_t bit = j - t.base;
        if (bit < 0 || bit >= 128) masks_ok = false;
        else {
            uint64_t &mw = bit < 64 ? t.mask : t.mask2;
            if (mw & (1ull << (bit & 63))) { RepStat &r = b.rep_host[k]; (bit < 64 ? r.rmask : r.rmask2) |= 1ull << (bit & 63); }
            mw |= 1ull << (bit & 63);
        }
    }
    b.n_all = n_all; b.kmin = kmin; b.kmax = kmax; b.f_lo = f_lo; b.E_own = E_own;
    b.sorted = sorted; b.masks_ok = masks_ok; b.mono_j = mono_j; b.src_ok = src_ok; b.any_self = any_self;
}

// the same figures from the device's table (bit b of a mask: target frame src - 64 + b)
int scan_device_table(PlanBuild &b) {
    const DevPlanStats *dstats = b.dstats;
    bt_plan *pl = b.pl;
    b.n_all = std::max(b.n_all, dstats->n_all); b.f_lo = dstats->f_lo; b.kmin = dstats->kmin; b.kmax = dstats->kmax;
    b.any_self = dstats->any_self != 0; b.sorted = false;
    // a sharded plan lays out the tracks of [own_lo, own_hi) only: the device's sort keeps a patch's edges together in
    // patch order, so the rank's edges are ONE segment of the sorted list — it starts behind the edges of the patches in
    // front of the range (dev_q0).  The other ranks' tracks keep their (source frame, mask) for the pattern of S below.
    // (round 6: the table of such a plan holds the rank's own patches only — dstats->sliced —, the edges in front of them, the
    //  tracks in front of them and the coupling pattern of the whole list come reduced from the device)
    pl->dev_q0 = dstats->sliced ? dstats->edges_before : 0;
    for (int64_t k = dstats->tab_lo; k < dstats->tab_lo + dstats->tab_n; ++k) {
        const PatchStat &d = dstats->tab[(size_t)(k - dstats->tab_lo)];
        PerPatch &t = b.pp[k];
        t.src = d.src; t.base = d.src - 64; t.last_j = 0; t.mask = d.mask; t.mask2 = d.mask2;
        if (k >= b.own_lo && k < b.own_hi) { t.cnt = d.cnt; b.E_own += d.cnt; }
        else { t.cnt = 0; if (k < b.own_lo) pl->dev_q0 += d.cnt; }
    }
    return b.E_own == 0 ? (int)BT_NEED_EDGES : (int)BT_OK;     // (a rank without tracks: nothing for the device passes to lay out)
}

// what follows from the pass: the sharded plan's track offset, the free poses, the kernels' tile thresholds for this plan
int edge_pass_figures(PlanBuild &b) {
    bt_plan *pl = b.pl;
    bt_plan_info &I = pl->info;
    const DevPlanStats *dstats = b.dstats;
    // sharded plan: the number of distinct tracks in front of this rank's range — a per-track lmbda tensor (ba.py:299-300) is
    // indexed by the GLOBAL track number, the kernels count from the rank's first track
    pl->dev.trk_off = 0;
    if (dstats) {
        if (dstats->sliced) pl->dev.trk_off = (int)dstats->trk_before;
        else for (int64_t k = b.kmin; k < std::min(b.own_lo, b.kmax + 1); ++k) pl->dev.trk_off += dstats->tab[(size_t)(k - dstats->tab_lo)].cnt > 0 ? 1 : 0;
    } else if (b.E_own != b.E && b.own_lo > 0) {
        std::vector<uint8_t> seen((size_t)b.own_lo, 0);
        for (int64_t e = 0; e < b.E; ++e) { const int64_t k = b.KK(e); if (k < b.own_lo && !seen[(size_t)k]) { seen[(size_t)k] = 1; ++pl->dev.trk_off; } }
    }
    pl->dev.em_self = b.any_self ? 1 : 0;
    if (b.E == 0) b.f_lo = 0;
    I.n_all = b.n_all;
    I.sorted_input = b.sorted ? 1 : 0;
    b.n = std::max<int64_t>(b.n_all - b.fixedp, 0);
    I.n = b.n;
    if (b.n > kMaxFreeWide) return BT_EUNSUPPORTED;          // (beyond kMaxFree: the dense solver, ba_dense.hip)
    if (!b.src_ok) return BT_EUNSUPPORTED;
    I.E = b.E_own;
    // Tile counts from which the wave-per-tile kernels take THIS plan.  A rank's plan of a sharded solve (own_lo / own_hi) holds
    // its share of the tiles: the thresholds shrink by that share, so that all ranks of a graph large enough for those kernels use
    // them (and the same per-edge precision), instead of a rank falling back to the float64 tile kernel because ITS shard is small.
    const auto shard_min = [&](int thr) {
        if (b.E_own >= b.E || thr <= 1 || thr >= (1 << 29)) return thr;
        return (int)std::max<int64_t>(1, ((int64_t)thr * b.E_own + b.E - 1) / b.E);
    };
    b.em_min_p = shard_min(edge_min_tiles()); b.st_min_p = shard_min(stream_min_tiles());
    return BT_OK;
}

// unique tracks, ascending (ba.py:276); off = first position of a track's edges in the grouped order.
// trk_of_patch is kept for the window only (trk_win[p - kmin]); bt_plan_array expands it on request.
void number_tracks(PlanBuild &b) {
    bt_plan *pl = b.pl;
    const DevPlanStats *dstats = b.dstats;
    const int64_t kmin = b.kmin, kmax = b.kmax;
    int32_t m = 0;
    pl->kx.clear();
    pl->trk_win_lo = kmin <= kmax ? kmin : 0;
    pl->k_hi = kmax;
    pl->trk_win.assign(kmin <= kmax ? (size_t)(kmax - kmin + 1) : 0, -1);
    std::vector<int32_t> &off = b.off;
    off.assign(1, 0);
    // (a rank's sliced table: only its own patches can carry a track of this plan)
    const int64_t p_first = dstats && dstats->sliced ? dstats->tab_lo : kmin, p_last = dstats && dstats->sliced ? dstats->tab_lo + dstats->tab_n - 1 : kmax;
    for (int64_t p = p_first; p <= p_last; ++p) {
        const int32_t c = b.pp[p].cnt;
        if (c > 0) { pl->kx.push_back((int32_t)p); off.push_back(off.back() + c); pl->trk_win[(size_t)(p - kmin)] = m++; }
    }
    b.m = m;
    pl->info.m = m;
}

// ---- distinct camera pairs, ascending (i, j); looked up through a table over the frames the edges name, [f_lo, n_all):
// the window (about 20 frames), not the keyframe count of the whole sequence
void number_pairs(PlanBuild &b) {
    bt_plan *pl = b.pl;
    const int64_t f_lo = b.f_lo, nw = b.nw = b.n_all - b.f_lo;
    std::vector<int32_t> &pair_of = b.pair_of;
    pair_of.assign((size_t)(nw * nw), -1);
    if (b.masks_ok) {
        // from the tracks' (source frame, target mask): a few thousand tracks instead of every edge
        // (neighbouring tracks mostly share their source frame and targets — the tracks of one frame: such a track adds nothing)
        // (the masks of a source frame's tracks are bits around the same base, src - 64: their union per frame, two words a track —
        //  a graph whose tracks all differ, observations missing at random, walked every target of a million tracks here)
        std::vector<uint64_t> fm((size_t)nw * 2, 0);
        for (int32_t k = 0; k < b.m; ++k) {
            const PerPatch &t = b.track(k);
            fm[(size_t)(t.src - f_lo) * 2] |= t.mask; fm[(size_t)(t.src - f_lo) * 2 + 1] |= t.mask2;
        }
        for (int64_t f = 0; f < nw; ++f) {
            int32_t *row = pair_of.data() + (size_t)f * nw - f_lo;
            for_targets(fm[(size_t)f * 2], fm[(size_t)f * 2 + 1], (int32_t)(f + f_lo) - 64, [&](int32_t fr) { row[fr] = 0; });
        }
    } else {
        for (int64_t e = 0; e < b.E; ++e) if (b.owned(e)) pair_of[(size_t)((b.II(e) - f_lo) * nw + (b.JJ(e) - f_lo))] = 0;
    }
    pl->pair_i.clear(); pl->pair_j.clear();
    for (int64_t key = 0; key < nw * nw; ++key)
        if (pair_of[(size_t)key] == 0) {
            pair_of[(size_t)key] = (int32_t)pl->pair_i.size();
            pl->pair_i.push_back((int32_t)(key / nw + f_lo));
            pl->pair_j.push_back((int32_t)(key % nw + f_lo));
        }
    pl->info.pairs = (int64_t)pl->pair_i.size();
}

// ---- edges grouped by track, ordered by (pair, original index) ---------
// Two stable counting passes instead of a sort per track: first by target frame, then by track.  Within a
// track the source frame is the same for all edges (checked above), so ascending target frame IS ascending
// pair id, and stability keeps the original index as the tie-break (duplicates are normal, batrack.py:399-410).
// (the packed words travel with the order — pks[q] = pk[ord[q]] — so that the per-tile walks below read the edges' frames
//  in sequence instead of through ord into the caller's order: those random reads were most of the 0.9 ms of the walks)
void group_edges(PlanBuild &b) {
    if (b.dstats) return;                       // (no edge is read: the order of a track's edges is the device's sort)
    const int64_t E = b.E, E_own = b.E_own;
    const uint64_t *pk = b.pk;
    std::vector<int32_t> &byj = scratch().byj;
    b.ord.resize((size_t)E_own + 1); byj.resize((size_t)E_own + 1); b.pks.resize((size_t)E_own + 1);
    int32_t *ord = b.ord.data();
    uint64_t *pks = b.pks.data();
    std::vector<int32_t> cur(b.off.begin(), b.off.end() - 1);
    if (b.mono_j) {
        // every track's edges already come in (target frame, index) order: one stable scatter by track
        for (int64_t e = 0; e < E; ++e)
            if (E_own == E || b.owned(e)) { const int32_t q = cur[(size_t)b.trk_of(b.KK(e))]++; ord[(size_t)q] = (int32_t)e; pks[(size_t)q] = pk[e]; }
    } else {
        std::vector<int32_t> &cj = b.cj;
        for (int64_t j = 0; j < b.n_all; ++j) cj[(size_t)j + 1] += cj[(size_t)j];
        if (E_own == E) {
            for (int64_t e = 0; e < E; ++e) byj[(size_t)cj[(size_t)b.JJ(e)]++] = (int32_t)e;
        } else {
            for (int64_t e = 0; e < E; ++e) if (b.owned(e)) byj[(size_t)cj[(size_t)b.JJ(e)]++] = (int32_t)e;
        }
        for (int64_t q = 0; q < E_own; ++q) {
            const int32_t e = byj[(size_t)q];
            const int32_t pos = cur[(size_t)b.trk_of(b.KK(e))]++;
            ord[(size_t)pos] = e; pks[(size_t)pos] = pk[e];
        }
    }
}

// ---- tiles: greedy over sorted tracks ----------------------------------
struct Tiler {
    std::vector<int32_t> tile_set;      // the free cameras of the open tile
    int32_t epoch = 0, trk0 = 0;        // its number among all tiles opened so far; its first track
};

void close_tile(PlanBuild &b, Tiler &tl, int32_t trk_end) {
    bt_plan *pl = b.pl;
    if (trk_end == tl.trk0) return;
    std::sort(tl.tile_set.begin(), tl.tile_set.end());
    const int32_t T = (int32_t)pl->tile_trk0.size();
    int32_t nslot = 0;
    for (int32_t k = tl.trk0; k < trk_end; ++k) {
        nslot = std::max(nslot, b.off[(size_t)k + 1] - b.off[(size_t)k]);
        pl->trk_loc[(size_t)k] = (T << 6) | (k - tl.trk0);
    }
    pl->tile_trk0.push_back(tl.trk0); pl->tile_ntrk.push_back(trk_end - tl.trk0);
    pl->tile_ncam.push_back((int32_t)tl.tile_set.size());
    pl->tile_cam0.push_back((int32_t)pl->tile_cams.size());
    pl->tile_cams.insert(pl->tile_cams.end(), tl.tile_set.begin(), tl.tile_set.end());
    pl->tile_slot0.push_back((int32_t)b.slots); pl->tile_nslot.push_back(nslot);
    pl->tile_erow0.push_back((int32_t)b.erows);
    b.slots += nslot; b.erows += 6 * (int64_t)tl.tile_set.size();
    b.max_cams = std::max(b.max_cams, (int)tl.tile_set.size());
    tl.tile_set.clear(); ++tl.epoch; tl.trk0 = trk_end;
}

// What this attempt lays out: tracks per tile, and whether the slots are aligned.
int choose_layout(PlanBuild &b) {
    // Tracks per tile: 64 (one per lane of k_tile), or 16 for the graphs of FEW tiles with DEEP edge lists per track — a sliding
    // window (batrack.py:399-410: ~2,500 tracks x ~54 edges) is 40 tiles of 64 tracks on a 256-CU part; the pair-major kernel
    // (k_etile) does not tie a lane to a track, so the same graph is spread over four times as many workgroups.  Plans whose
    // tiles turn out not to fit that kernel are rebuilt with 64 (kRelayoutLargeTiles).
    const int32_t m = b.m;
    b.tcap = kLanes;
    {
        const int pm_env = etile_mode();
        const int64_t t64 = (m + kLanes - 1) / kLanes;
        if (pm_env && b.lay.small_tiles_allowed && t64 > 0 && t64 <= 96 && b.E_own >= 24 * (int64_t)m && t64 < std::min(b.em_min_p, b.st_min_p) / 4) b.tcap = 16;
    }
    if (b.dstats && b.tcap == kLanes) {                            // the device then writes the [slots][64] arrays and the wave cuts
        if (etile_mode() == 2) return BT_NEED_EDGES;                    // (pair-major tables of 64-track tiles are made from the host's slot arrays)
    }
    // ALIGNED SLOTS (round 6) for the plans the wave-per-tile kernels take.  k_edge2 / k_edge2u need every tile SLOT-UNIFORM — all
    // tracks of a tile with the same camera pair (or no edge) in slot s.  With slot s = a track's s-th edge that holds only where
    // all tracks of a tile have the same observations: one missing observation shifts the rest of its track (a graph with a random
    // 15 % of its observations dropped fell to k_stream: three times the time per edge).  So a tile's slots are laid out per PAIR:
    // local pair p gets mult[p] consecutive slots from pbase[p], mult[p] = the largest number of edges a track of the tile has (or,
    // from the tracks' figures alone, can have) with that pair; a track's r-th edge with pair p sits in slot pbase[p] + r, the
    // slots it does not fill are null (edge -1: zero weight in every kernel).  Every tile is then slot-uniform by construction at
    // sum(mult) slots instead of the longest track's count — 1 / (1 - drop) of the uniform cost.  Tiles do not run across two
    // source frames (the pairs of one are no pairs of the other; the kernels also take a tile's source camera from its first track).
    // Where it does not fit (more than 64 slots in some tile) the plan is laid out again the old way (kRelayoutUnaligned).
    b.aligned = b.lay.aligned_allowed && b.masks_ok && b.tcap == kLanes && m > 0 && ((int64_t)m + kLanes - 1) / kLanes >= b.em_min_p &&
                (!b.dstats || b.dstats->rep_known);
    return BT_OK;
}

// Aligned layout: the same greedy rule as tile_tracks on bit masks (a tile has one source frame, so its tracks' masks share their
// base): cameras = the free frames among the targets and the source frame (bit 64), in ascending order as the bits are
int tile_tracks_aligned(PlanBuild &b, Tiler &tl) {
    bt_plan *pl = b.pl;
    const int64_t fixedp = b.fixedp;
    const int tcap = b.tcap, cam_hard = b.lay.cam_hard;
    int32_t cur_src = -1;
    uint64_t free_lo = 0, free_hi = 0, tm_lo = 0, tm_hi = 0, tg_lo = 0, tg_hi = 0, pm_lo = ~0ull, pm_hi = ~0ull;
    auto flush = [&](int32_t k_end) {
        if (k_end == tl.trk0) return;
        tl.tile_set.clear();
        for_targets(tm_lo, tm_hi, cur_src - 64, [&](int32_t fr) { tl.tile_set.push_back((int32_t)(fr - fixedp)); });
        b.tile_tmask.push_back(tg_lo); b.tile_tmask.push_back(tg_hi);
        close_tile(b, tl, k_end);
        tm_lo = tm_hi = tg_lo = tg_hi = 0;
    };
    for (int32_t k = 0; k < b.m; ++k) {
        const PerPatch &t = b.track(k);
        if (t.src != cur_src) {
            flush(k);
            cur_src = t.src; pm_lo = pm_hi = ~0ull;
            const int64_t first_free = fixedp - ((int64_t)t.src - 64);          // bits >= this are free frames
            free_lo = first_free <= 0 ? ~0ull : first_free >= 64 ? 0ull : ~0ull << first_free;
            free_hi = first_free <= 64 ? ~0ull : first_free >= 128 ? 0ull : ~0ull << (first_free - 64);
        }
        if (k > tl.trk0 && k - tl.trk0 < tcap && t.mask == pm_lo && t.mask2 == pm_hi) continue;      // (the same targets as the track before: nothing new)
        pm_lo = t.mask; pm_hi = t.mask2;
        const uint64_t c_lo = t.mask & free_lo, c_hi = (t.mask2 & free_hi) | (t.src >= fixedp ? 1ull : 0ull);
        const int nk = __builtin_popcountll(c_lo) + __builtin_popcountll(c_hi);
        if (nk > cam_hard) {                                   // a loose track (see tile_tracks)
            if (b.dstats) return BT_NEED_EDGES;
            flush(k);
            b.loose.push_back(k);
            pl->trk_loc[(size_t)k] = -1;
            tl.trk0 = k + 1;
            continue;
        }
        const int add = __builtin_popcountll(c_lo & ~tm_lo) + __builtin_popcountll(c_hi & ~tm_hi);
        const int have = __builtin_popcountll(tm_lo) + __builtin_popcountll(tm_hi);
        if (k - tl.trk0 >= tcap || (k > tl.trk0 && have + add > std::max<int>(kTileCamSoft, nk))) flush(k);
        tm_lo |= c_lo; tm_hi |= c_hi; tg_lo |= t.mask; tg_hi |= t.mask2;
    }
    flush(b.m);
    return BT_OK;
}

// The general layout: a tile takes tracks while the union of their free cameras stays within kTileCamSoft (or one track's own
// count) and its pairs within kMaxTilePairs.
// LOOSE tracks: seen by more free cameras than a tile takes.  64 is what the kernels' tables take (kTileCamHard) — but a tile of
// more than 32 cameras no longer holds its E in LDS as double, and ONE such tile turns the whole plan's per-edge maths to float32
// (bt_plan_edge_precision).  A landmark seen from 40 or 60 frames next to ordinary tracks — a handful per plan — is therefore
// loose as well (ba_loose.hip walks it in double; the plan stays float64: update errors 1e-6 instead of 1e-4 .. 1e-3 on such
// graphs, tests/test_gpu_fuzz.py); a plan with MANY tracks that long (more than kFewHubs) keeps them in tiles — there the loose
// path's atomics would cost more than float32 does — and is laid out again with the threshold at 64 (kRelayoutHubsInTiles).
int tile_tracks(PlanBuild &b, Tiler &tl) {
    bt_plan *pl = b.pl;
    const int64_t fixedp = b.fixedp;
    const bool masks_ok = b.masks_ok;
    const int tcap = b.tcap;
    const std::vector<int32_t> &off = b.off;
    std::vector<int32_t> stamp((size_t)b.n + 1, -1);      // last tile-epoch that contains camera c
    std::vector<int32_t> tstamp((size_t)b.n + 1, -1);     // last track that contains camera c
    std::vector<int32_t> trk_set;
    int32_t src_p = -1, base_p = 0, set_epoch = -1; uint64_t mask_p = 0, mask2_p = 0;         // the previous track's figures: the same again = the same cameras
    // A tile's camera PAIRS (source frame -> target frame, the fixed frames too: every pair's geometry sits in the tile's LDS table)
    // are bounded as well: kMaxTilePairs.  The cameras bound them only among the FREE frames — with most of a long trajectory fixed,
    // 64 tracks of few free cameras each name hundreds of pairs.  Counted per run of tracks with one source frame (tracks come
    // sorted by patch and a frame's patches are neighbours; a source frame that comes back counts again: the bound may close a
    // tile early, never late).
    std::vector<int32_t> pair_stamp((size_t)b.n_buf, -1);
    int32_t pair_run = 0, run_src = -1;
    int tile_pairs = 0;
    auto mark_targets = [&](int32_t k) -> int {                    // the track's targets not yet seen in this run (and now seen)
        int cnt = 0;
        auto mark = [&](int64_t fr) { if (pair_stamp[(size_t)fr] != pair_run) { pair_stamp[(size_t)fr] = pair_run; ++cnt; } };
        if (masks_ok) {
            const PerPatch &t = b.track(k);
            for_targets(t.mask, t.mask2, t.base, mark);
        } else {
            for (int32_t sidx = off[(size_t)k]; sidx < off[(size_t)k + 1]; ++sidx) mark(b.JQ(sidx));
        }
        return cnt;
    };
    for (int32_t k = 0; k < b.m; ++k) {
        if (masks_ok && k > 0 && b.same_targets(b.track(k), src_p, base_p, mask_p, mask2_p)) {
            // (trk_set is the previous track's and still right; in the tile it went into, it adds nothing)
            if (set_epoch == tl.epoch && k - tl.trk0 < tcap) continue;
        } else {
            trk_set.clear();
            auto see = [&](int64_t c) { if (c >= 0 && tstamp[(size_t)c] != k) { tstamp[(size_t)c] = k; trk_set.push_back((int32_t)c); } };
            if (masks_ok) {
                // the track's free cameras from its source frame and target mask (no walk over its edges)
                const PerPatch &t = b.track(k);
                src_p = t.src; base_p = t.base; mask_p = t.mask; mask2_p = t.mask2;
                see((int64_t)t.src - fixedp);
                for_targets(t.mask, t.mask2, t.base, [&](int32_t fr) { see((int64_t)fr - fixedp); });
            } else {
                for (int32_t sidx = off[(size_t)k]; sidx < off[(size_t)k + 1]; ++sidx) { see(b.IQ(sidx) - fixedp); see(b.JQ(sidx) - fixedp); }
            }
        }
        const int32_t src_k = masks_ok ? b.track(k).src : (int32_t)b.IQ(off[(size_t)k]);
        if (src_k != run_src) { run_src = src_k; ++pair_run; }
        int np_new = mark_targets(k);
        bool too_many_pairs = false;                               // (the track alone: possible only without masks — they hold 128 targets)
        if (!masks_ok && off[(size_t)k + 1] - off[(size_t)k] > kMaxTilePairs) { ++pair_run; too_many_pairs = mark_targets(k) > kMaxTilePairs; }
        if ((int)trk_set.size() > b.lay.cam_hard || too_many_pairs) {
            // a LOOSE track: in no tile (its E does not fit a tile's camera budget, or its pairs a tile's table); ba_loose.hip walks its edges
            if (b.dstats) return BT_NEED_EDGES;                    // (their edge lists come from the host's grouped order)
            // (k_etile's stored per-tile sums have no place for them: 64-track tiles, atomics)
            if (tcap < kLanes) return b.lay.small_tiles_allowed ? (int)kRelayoutLargeTiles : (int)BT_EUNSUPPORTED;
            close_tile(b, tl, k);
            b.loose.push_back(k);
            pl->trk_loc[(size_t)k] = -1;
            tl.trk0 = k + 1;
            src_p = -1;                                            // (the next track starts a tile: its cameras are looked at afresh)
            tile_pairs = 0; ++pair_run;
            continue;
        }
        int add = 0;
        for (int32_t c : trk_set) if (stamp[(size_t)c] != tl.epoch) ++add;
        const int limit = std::max<int>(kTileCamSoft, (int)trk_set.size());
        if (k - tl.trk0 >= tcap || (k > tl.trk0 && ((int)tl.tile_set.size() + add > limit || tile_pairs + np_new > kMaxTilePairs))) {
            close_tile(b, tl, k);
            tile_pairs = 0; ++pair_run;
            np_new = mark_targets(k);                              // (all of the track's pairs are new to the tile it opens)
        }
        tile_pairs += np_new;
        for (int32_t c : trk_set) if (stamp[(size_t)c] != tl.epoch) { stamp[(size_t)c] = tl.epoch; tl.tile_set.push_back(c); }
        set_epoch = tl.epoch;
    }
    close_tile(b, tl, b.m);
    return BT_OK;
}

// ---- per tile: its distinct camera pairs (their relative pose is computed once per tile), then the slot arrays
// [slots][64] with the local pair index of every edge, in one walk over the tile's edges
// (a plan tiled for k_etile — tcap < 64 — gets its pair-major tables straight from the tracks' edge lists here; the
//  [slots][64] arrays of k_tile, three quarters of them padding at 16 tracks per tile, are then built only on request:
//  host-only plans, which the tests' emulator executes)
struct TileWalk {
    int32_t t = 0, t0 = 0, nt = 0, ns_t = 0;                        // the tile, its first track, its tracks, its slots
    std::vector<int32_t> local, lp_of, mine, mult, pbase, pm_cnt;  // local camera of a free camera / local pair of a pair; the tile's pairs
    std::vector<uint8_t> crossed;                                  // crossed[s]: some track's run spans slots s - 1 and s
    int64_t slots_al = 0;                                          // aligned layout: the slots of the tiles so far
};

// the tile's pairs, ascending, and lp_of for them
int tile_pair_list(PlanBuild &b, TileWalk &w) {
    std::vector<int32_t> &mine = w.mine, &lp_of = w.lp_of;
    const auto add_pair = [&](int32_t gp) { if (lp_of[(size_t)gp] < 0) { lp_of[(size_t)gp] = 0; mine.push_back(gp); } };
    mine.clear();
    if (b.aligned) {
        // (one source frame per tile: its pairs are (source, target) over the union of the tracks' target masks, ascending)
        const int32_t src_t = b.track(w.t0).src;
        const int32_t *row = b.pair_row(src_t);
        for_targets(b.tile_tmask[(size_t)w.t * 2], b.tile_tmask[(size_t)w.t * 2 + 1], src_t - 64, [&](int32_t fr) { mine.push_back(row[fr]); });
        for (int32_t gp : mine) lp_of[(size_t)gp] = 0;
    } else if (b.masks_ok) {
        int32_t src_b = -1, base_b = 0; uint64_t mask_b = 0, mask2_b = 0;
        for (int32_t l = 0; l < w.nt; ++l) {
            const PerPatch &tp = b.track(w.t0 + l);
            if (b.same_targets(tp, src_b, base_b, mask_b, mask2_b)) continue;       // (the same pairs as the track before)
            src_b = tp.src; base_b = tp.base; mask_b = tp.mask; mask2_b = tp.mask2;
            const int32_t *row = b.pair_row(tp.src);
            for_targets(tp.mask, tp.mask2, tp.base, [&](int32_t fr) { add_pair(row[fr]); });
        }
    } else {
        for (int32_t q = b.off[(size_t)w.t0]; q < b.off[(size_t)(w.t0 + w.nt)]; ++q) add_pair(b.pair_q(q));
    }
    std::sort(mine.begin(), mine.end());
    if ((int)mine.size() > kMaxTilePairs) return BT_EUNSUPPORTED;
    for (size_t q = 0; q < mine.size(); ++q) lp_of[(size_t)mine[q]] = (int32_t)q;
    return BT_OK;
}

// aligned layout: the slots of every pair of the tile (mult) and the first of them (pbase); the tile's slot count with them
int aligned_slot_bases(PlanBuild &b, TileWalk &w) {
    bt_plan *pl = b.pl;
    const DevPlanStats *dstats = b.dstats;
    // slots per pair from the tracks' figures (no edge is read): a target outside the track's repeat mask has one
    // edge; the repeated ones share the track's surplus, cnt - (distinct targets), each holding at least one of it
    // (every pair of the tile has a slot; only the tracks that repeat a target are looked at bit by bit)
    w.mult.assign(w.mine.size(), 1);
    for (int32_t l = 0; l < w.nt; ++l) {
        const PerPatch &tp = b.track(w.t0 + l);
        const int32_t distinct = __builtin_popcountll(tp.mask) + __builtin_popcountll(tp.mask2);
        if (tp.cnt <= distinct) continue;
        RepStat rs{0, 0};
        const int64_t patch = pl->kx[(size_t)(w.t0 + l)];
        if (dstats) { if (dstats->rtab) rs = dstats->rtab[(size_t)(patch - dstats->tab_lo)]; }
        else { const auto it = b.rep_host.find(patch); if (it != b.rep_host.end()) rs = it->second; }
        rs.rmask &= tp.mask; rs.rmask2 &= tp.mask2;
        const int32_t nrep = __builtin_popcountll(rs.rmask) + __builtin_popcountll(rs.rmask2);
        if (nrep == 0) { pl->dev_pbase.clear(); return BT_EINVAL; }      // (cannot happen: a surplus edge repeats some target)
        const int32_t mrep = 1 + (tp.cnt - distinct) - (nrep - 1);
        const int32_t *row = b.pair_row(tp.src);
        for_targets(rs.rmask, rs.rmask2, tp.base, [&](int32_t fr) {
            int32_t &mu = w.mult[(size_t)w.lp_of[(size_t)row[fr]]];
            mu = std::max(mu, mrep);
        });
    }
    w.pbase.assign(w.mine.size(), 0);
    int32_t acc = 0;
    for (size_t q = 0; q < w.mine.size(); ++q) { w.pbase[q] = acc; acc += w.mult[q]; }
    // (more (pair, repeat) slots than an iteration has lanes: the edge-major layout does not hold this tile)
    if (acc > kLanes) return kRelayoutUnaligned;
    w.ns_t = acc;
    pl->tile_slot0[(size_t)w.t] = (int32_t)w.slots_al; pl->tile_nslot[(size_t)w.t] = w.ns_t;
    w.slots_al += w.ns_t;
    pl->dev_pbase.insert(pl->dev_pbase.end(), w.pbase.begin(), w.pbase.end());
    w.crossed.assign((size_t)w.ns_t + 1, 0);
    if (b.want_slots) {
        pl->slot_edge.resize((size_t)w.slots_al * kLanes, -1); pl->slot_pair.resize((size_t)w.slots_al * kLanes, 0);
        pl->slot_lab.resize((size_t)w.slots_al * kLanes, 0xffff); pl->slot_lp.resize((size_t)w.slots_al * kLanes, 0);
    }
    return BT_OK;
}

// pair-major tables of this tile (layout: pair_major_tables, which builds them from the slot arrays)
void pair_major_tile(PlanBuild &b, TileWalk &w) {
    bt_plan *pl = b.pl;
    const int64_t fixedp = b.fixedp;
    const int32_t t = w.t, t0 = w.t0, nt = w.nt, np = (int32_t)w.mine.size();
    const std::vector<int32_t> &off = b.off, &local = w.local;
    if (np > kLanes) { b.pm_fail = true; return; }
    const int lg = ceil_log2(np);
    const int32_t S = 1 << lg, G = kLanes >> lg, nit = (nt + G - 1) / G;
    if (b.dstats) {
        // the tile's record but for its rounds, the local target camera of its pairs and the local source camera
        // of its tracks; the table itself and the rounds come from the device
        pl->pm_rec[(size_t)t * 4 + 1] = lg;
        pl->pm_rec[(size_t)t * 4 + 2] = nit;
        for (int32_t q = 0; q < np; ++q) {
            const int64_t b2 = (int64_t)pl->pair_j[(size_t)w.mine[(size_t)q]] - fixedp;
            pl->pm_lb[(size_t)t * kLanes + (size_t)q] = b2 >= 0 ? (uint8_t)local[(size_t)b2] : (uint8_t)0xff;
        }
        for (int32_t l = 0; l < nt; ++l) {
            const int64_t a2 = (int64_t)b.track(t0 + l).src - fixedp;
            pl->pm_la[(size_t)t * kLanes + (size_t)l] = a2 >= 0 ? (uint8_t)local[(size_t)a2] : (uint8_t)0xff;
        }
        return;
    }
    std::vector<uint32_t> &pm_code = scratch().pm_code;
    w.pm_cnt.assign((size_t)nt * (size_t)S, 0);
    // one walk over the tile's edges (each a random access into the packed edge list): local pair, local
    // cameras and the round of every edge; the table is filled from these codes
    const int32_t q0 = off[(size_t)t0], q1 = off[(size_t)(t0 + nt)];
    pm_code.resize((size_t)(q1 - q0));
    int32_t D = 1;
    for (int32_t l = 0; l < nt; ++l)
        for (int32_t sidx = off[(size_t)(t0 + l)]; sidx < off[(size_t)(t0 + l) + 1]; ++sidx) {
            const int64_t i = b.IQ(sidx), j = b.JQ(sidx), a2 = i - fixedp, b2 = j - fixedp;
            const int32_t lp = w.lp_of[(size_t)b.pair_ij(i, j)];
            const int32_t d = w.pm_cnt[(size_t)l * S + lp]++;
            D = std::max(D, d + 1);
            const uint32_t la = a2 >= 0 ? (uint32_t)local[(size_t)a2] : 0xffu, lb = b2 >= 0 ? (uint32_t)local[(size_t)b2] : 0xffu;
            pm_code[(size_t)(sidx - q0)] = (uint32_t)lp | (la << 8) | (lb << 16) | ((uint32_t)std::min(d, 255) << 24);
        }
    if (D > 255) { b.pm_fail = true; return; }
    pl->pm_rec[(size_t)t * 4] = (int32_t)b.pm_rounds_acc;
    pl->pm_rec[(size_t)t * 4 + 1] = lg | (D << 8);
    pl->pm_rec[(size_t)t * 4 + 2] = nit;
    pl->pm_edge.resize((size_t)(b.pm_rounds_acc + (int64_t)nit * D) * kLanes, -1);
    for (int32_t l = 0; l < nt; ++l)
        for (int32_t sidx = off[(size_t)(t0 + l)]; sidx < off[(size_t)(t0 + l) + 1]; ++sidx) {
            const uint32_t c = pm_code[(size_t)(sidx - q0)];
            const int32_t lp = (int32_t)(c & 0xffu), d = (int32_t)(c >> 24);
            pl->pm_edge[pm_index(b.pm_rounds_acc, l, G, D, d, lg, lp)] = b.ord[(size_t)sidx];
            pl->pm_lb[(size_t)t * kLanes + (size_t)lp] = (uint8_t)((c >> 16) & 0xffu);
            pl->pm_la[(size_t)t * kLanes + (size_t)l] = (uint8_t)((c >> 8) & 0xffu);
        }
    b.pm_rounds_acc += (int64_t)nit * D;
}

// the tile's rows of the slot arrays: edge, pair, local cameras and local pair of every (slot, lane)
void slot_rows(PlanBuild &b, TileWalk &w) {
    bt_plan *pl = b.pl;
    const int64_t fixedp = b.fixedp;
    for (int32_t l = 0; l < w.nt; ++l) {
        const int32_t k = w.t0 + l;
        uint16_t lb_before = 0xff;
        int32_t gp_before = -1, rank = 0;                  // aligned layout: the edge's rank among the track's edges with its pair
        for (int32_t sidx = b.off[(size_t)k]; sidx < b.off[(size_t)k + 1]; ++sidx) {
            const int32_t e = b.ord[(size_t)sidx];
            const int64_t i = b.IQ(sidx), j = b.JQ(sidx);
            const int64_t a = i - fixedp, bb = j - fixedp;
            const uint16_t la = a >= 0 ? (uint16_t)w.local[(size_t)a] : 0xff;
            const uint16_t lb = bb >= 0 ? (uint16_t)w.local[(size_t)bb] : 0xff;
            const int32_t gp = b.pair_ij(i, j);
            rank = gp == gp_before ? rank + 1 : 0;
            gp_before = gp;
            const int32_t sl = b.aligned ? w.pbase[(size_t)w.lp_of[(size_t)gp]] + rank : sidx - b.off[(size_t)k];
            const size_t idx = ((size_t)pl->tile_slot0[(size_t)w.t] + (size_t)sl) * kLanes + (size_t)l;
            pl->slot_edge[idx] = e;
            pl->slot_pair[idx] = gp;
            pl->slot_lab[idx] = (uint16_t)(la | (lb << 8));
            pl->slot_lp[idx] = (uint8_t)w.lp_of[(size_t)gp];
            if (lb != 0xff && lb == lb_before) w.crossed[(size_t)sl] = 1;
            lb_before = lb;
        }
    }
}

// tile_cut8 / tile_cut16: where k_tile's 8 or 16 waves split the tile's slots.  Repeated observations of one (track,
// target camera) are consecutive slots of that track; a wave sums such a run in registers and writes it once, but a run
// that continues into the next wave's chunk forces LDS float atomics on every slot of it (~500 cycles per wave
// instruction on this part).  The sliding-window caller repeats observations all the time and all tracks of a tile
// share their pattern, so the cuts are moved to the nearest slot boundary that no track's run crosses.
void wave_cuts(PlanBuild &b, const TileWalk &w) {
    bt_plan *pl = b.pl;
    const int32_t ns_t = w.ns_t;
    const std::vector<uint8_t> &crossed = w.crossed;
    for (int W = 8; W <= 16; W += 8) {
        uint16_t *cut = (W == 8 ? pl->tile_cut8.data() + (size_t)w.t * 9 : pl->tile_cut16.data() + (size_t)w.t * 17);
        const int32_t chunk = (ns_t + W - 1) / W;
        int32_t prev = 0;
        cut[0] = 0;
        for (int wv = 1; wv < W; ++wv) {
            const int32_t ideal = std::min(ns_t, wv * chunk);
            int32_t best = ideal;
            if (ideal < ns_t && crossed[(size_t)ideal]) {          // nearest uncrossed boundary within a chunk's reach, else keep it
                for (int32_t d = 1; d <= chunk; ++d) {
                    if (ideal - d >= prev && !crossed[(size_t)(ideal - d)]) { best = ideal - d; break; }
                    if (ideal + d <= ns_t && (ideal + d == ns_t || !crossed[(size_t)(ideal + d)])) { best = ideal + d; break; }
                }
            }
            best = std::max(best, prev);
            cut[wv] = (uint16_t)best;
            prev = best;
        }
        cut[W] = (uint16_t)ns_t;
    }
}

int fill_tiles(PlanBuild &b) {
    bt_plan *pl = b.pl;
    bt_plan_info &I = pl->info;
    const int32_t T = (int32_t)I.tiles;
    b.dev_slots = b.dstats && b.tcap == kLanes;            // the slot arrays are written on the device (plan_device.hip)
    b.want_slots = (b.tcap == kLanes || b.keep_slots) && !b.dev_slots;
    b.pm_direct = b.tcap < kLanes;
    b.pm_fail = false;
    b.pm_rounds_acc = 0;
    if (b.pm_direct) {
        pl->pm_rec.assign((size_t)T * 4, 0);
        pl->pm_lb.assign((size_t)T * kLanes, 0xff);
        pl->pm_la.assign((size_t)T * kLanes, 0xff);
        pl->pm_edge.clear();
        pl->pm_edge.reserve((size_t)b.E_own * 2 + (size_t)T * kLanes * 4);      // (one allocation: the table grows tile by tile)
    }
    const size_t slot_elems = b.want_slots && !b.aligned ? (size_t)b.slots * kLanes : 0;      // (aligned: the arrays grow tile by tile below)
    pl->slot_edge.assign(slot_elems, -1);
    pl->slot_pair.assign(slot_elems, 0);
    pl->slot_lab.assign(slot_elems, 0xffff);
    pl->slot_lp.assign(slot_elems, 0);
    pl->tile_pair0.assign((size_t)T, 0); pl->tile_npair.assign((size_t)T, 0);
    pl->tile_pairs.clear();
    pl->dev.max_tile_pairs = 0;
    pl->tile_cut8.assign((size_t)T * 9, 0);
    pl->tile_cut16.assign((size_t)T * 17, 0);
    TileWalk w;
    w.local.assign((size_t)b.n + 1, -1); w.lp_of.assign(pl->pair_i.size(), -1);
    for (int32_t t = 0; t < T; ++t) {
        const int32_t c0 = pl->tile_cam0[(size_t)t], nc = pl->tile_ncam[(size_t)t];
        w.t = t; w.t0 = pl->tile_trk0[(size_t)t]; w.nt = pl->tile_ntrk[(size_t)t]; w.ns_t = pl->tile_nslot[(size_t)t];
        if (w.ns_t > 0xffff) return BT_EUNSUPPORTED;           // (a track with more than 65535 observations)
        if (!b.aligned) w.crossed.assign((size_t)w.ns_t + 1, 0);
        for (int32_t c = 0; c < nc; ++c) w.local[(size_t)pl->tile_cams[(size_t)(c0 + c)]] = c;
        int rc = tile_pair_list(b, w);
        if (rc == BT_OK && b.aligned) rc = aligned_slot_bases(b, w);
        if (rc != BT_OK) return rc;
        if (b.pm_direct && !b.pm_fail) pair_major_tile(b, w);
        if (b.want_slots) { slot_rows(b, w); wave_cuts(b, w); }
        pl->tile_pair0[(size_t)t] = (int32_t)pl->tile_pairs.size();
        pl->tile_npair[(size_t)t] = (int32_t)w.mine.size();
        pl->tile_pairs.insert(pl->tile_pairs.end(), w.mine.begin(), w.mine.end());
        pl->dev.max_tile_pairs = std::max(pl->dev.max_tile_pairs, (int)w.mine.size());
        for (int32_t q : w.mine) w.lp_of[(size_t)q] = -1;
    }
    if (b.aligned) {
        int64_t tot = 0;
        for (int32_t t = 0; t < T; ++t) tot += pl->tile_nslot[(size_t)t];
        b.slots = tot; I.slots = tot;
    }
    return BT_OK;
}

void loose_lists_and_tile_flags(PlanBuild &b) {
    bt_plan *pl = b.pl;
    const int32_t T = (int32_t)pl->info.tiles;
    // the loose tracks' edge lists (grouped order: by pair, then by the caller's index) with their camera pairs
    pl->lz_trk.clear(); pl->lz_ptr.assign(1, 0); pl->lz_edge.clear(); pl->lz_pair.clear();
    for (int32_t k : b.loose) {
        pl->lz_trk.push_back(k);
        for (int32_t q = b.off[(size_t)k]; q < b.off[(size_t)k + 1]; ++q) { pl->lz_edge.push_back(b.ord[(size_t)q]); pl->lz_pair.push_back(b.pair_q(q)); }
        pl->lz_ptr.push_back((int32_t)pl->lz_edge.size());
    }
    // consecutive tiles with identical camera / pair lists: a persistent workgroup keeps its
    // accumulators across them
    pl->tile_flags.assign((size_t)T, 0);
    for (int32_t t = 1; t < T; ++t) {
        const int32_t nc = pl->tile_ncam[(size_t)t], np2 = pl->tile_npair[(size_t)t];
        if (nc == pl->tile_ncam[(size_t)t - 1] &&
            std::equal(pl->tile_cams.begin() + pl->tile_cam0[(size_t)t], pl->tile_cams.begin() + pl->tile_cam0[(size_t)t] + nc,
                       pl->tile_cams.begin() + pl->tile_cam0[(size_t)t - 1]))
            pl->tile_flags[(size_t)t] |= 1;
        if (np2 == pl->tile_npair[(size_t)t - 1] &&
            std::equal(pl->tile_pairs.begin() + pl->tile_pair0[(size_t)t], pl->tile_pairs.begin() + pl->tile_pair0[(size_t)t] + np2,
                       pl->tile_pairs.begin() + pl->tile_pair0[(size_t)t - 1]))
            pl->tile_flags[(size_t)t] |= 2;
    }
}

// ---- k_tile's first loads, indexed by the tile alone (no dependent index chain in its prologue):
//   tile_ij[t][max_tile_pairs]   cameras (i | j << 16) of the tile's pairs, in local pair order
//   tile_kx[t][64]               patch of every track of the tile (-1: no track in this lane)
void tile_first_loads(bt_plan *pl) {
    const bt_plan_info &I = pl->info;
    const size_t mtp = (size_t)std::max(pl->dev.max_tile_pairs, 1);
    pl->tile_ij.assign((size_t)I.tiles * mtp, 0);
    pl->tile_kx.assign((size_t)I.tiles * kLanes, -1);
    for (int64_t t = 0; t < I.tiles; ++t) {
        for (int32_t q = 0; q < pl->tile_npair[(size_t)t]; ++q) {
            const int32_t gp = pl->tile_pairs[(size_t)(pl->tile_pair0[(size_t)t] + q)];
            pl->tile_ij[(size_t)t * mtp + (size_t)q] = pl->pair_i[(size_t)gp] | (pl->pair_j[(size_t)gp] << 16);
        }
        for (int32_t ln = 0; ln < pl->tile_ntrk[(size_t)t]; ++ln)
            pl->tile_kx[(size_t)t * kLanes + (size_t)ln] = pl->kx[(size_t)(pl->tile_trk0[(size_t)t] + ln)];
    }
}

// tile_rec[t][0 .. 5] (stream_tables); straddle: 4 or 0, the record's flag bit 2
void fill_tile_rec(bt_plan *pl, int64_t t, int32_t straddle) {
    int32_t *r = pl->tile_rec.data() + (size_t)t * 8;
    r[0] = pl->tile_ntrk[(size_t)t] | (pl->tile_ncam[(size_t)t] << 8) | (pl->tile_npair[(size_t)t] << 16) | ((pl->tile_flags[(size_t)t] | straddle) << 24);
    r[1] = pl->tile_slot0[(size_t)t]; r[2] = pl->tile_nslot[(size_t)t]; r[3] = pl->tile_cam0[(size_t)t];
    r[4] = pl->tile_pair0[(size_t)t]; r[5] = pl->tile_trk0[(size_t)t];
}

// ---- compact tables of the wave-per-tile kernels (k_stream): per (slot, lane) a 16-bit code
// (local target camera | local pair << 8; the global pair id is tile_pairs[pair0 + local pair]); per (tile,
// lane) the local source camera (one per track: ii = ix[kk], checked above); per tile one 32-byte record
//   [0] ntrk | ncam << 8 | npair << 16 | flags << 24   [1] slot0  [2] nslot  [3] cam0  [4] pair0  [5] trk0
void stream_tables(PlanBuild &b) {
    bt_plan *pl = b.pl;
    const bt_plan_info &I = pl->info;
    b.want_stream_tables = b.want_slots && I.tiles >= std::min(b.em_min_p, b.st_min_p);   // (they are made from the slot arrays)
    b.dev_wpt = b.dev_slots && I.tiles >= std::min(b.em_min_p, b.st_min_p);               // (... where those are: on the device)
    pl->dev.st_ok = b.want_stream_tables || b.dev_wpt ? 1 : 0;
    pl->dev.st_min = b.st_min_p; pl->dev.em_min = b.em_min_p;
    pl->dev_wpt = b.dev_wpt ? 1 : 0;
    if (b.dev_wpt) {
        // the records but for the straddle flag (k_plan_slots adds it); slot_code, tile_la, it_edge and tile_sinfo are written
        // by the device's passes into the plan's buffer (plan_device.hip)
        pl->slot_code.clear(); pl->tile_la.clear(); pl->it_edge.clear(); pl->tile_sinfo.clear();
        pl->tile_rec.assign((size_t)I.tiles * 8, 0);
        for (int64_t t = 0; t < I.tiles; ++t) fill_tile_rec(pl, t, 0);
    }
    if (!b.want_stream_tables) return;
    pl->slot_code.assign((size_t)b.slots * kLanes, 0xffff);
    pl->tile_la.assign((size_t)I.tiles * kLanes, 0xff);
    pl->tile_rec.assign((size_t)I.tiles * 8, 0);
    for (int64_t t = 0; t < I.tiles; ++t) {
        const size_t b0 = (size_t)pl->tile_slot0[(size_t)t] * kLanes;
        const int32_t ns = pl->tile_nslot[(size_t)t];
        for (int32_t sl = 0; sl < ns; ++sl)
            for (int ln = 0; ln < kLanes; ++ln) {
                const size_t i = b0 + (size_t)sl * kLanes + (size_t)ln;
                if (pl->slot_edge[i] < 0) continue;
                pl->slot_code[i] = (uint16_t)((pl->slot_lab[i] >> 8) | ((uint16_t)pl->slot_lp[i] << 8));
                pl->tile_la[(size_t)t * kLanes + (size_t)ln] = (uint8_t)(pl->slot_lab[i] & 0xff);
            }
        // flag bit 2: some track repeats a target camera across the boundary of the two half-chunks of slots the
        // streaming kernel gives its two waves (both then add to the same element of the local E)
        int32_t straddle = 0;
        const int32_t ch = (ns + 1) >> 1;
        if (ch < ns)
            for (int ln = 0; ln < kLanes && !straddle; ++ln) {
                const size_t i0 = b0 + (size_t)(ch - 1) * kLanes + (size_t)ln, i1 = i0 + kLanes;
                if (pl->slot_edge[i0] >= 0 && pl->slot_edge[i1] >= 0 && (pl->slot_lab[i0] >> 8) != 0xff &&
                    (pl->slot_lab[i0] >> 8) == (pl->slot_lab[i1] >> 8)) straddle = 4;
            }
        fill_tile_rec(pl, t, straddle);
    }
}

// Per tile of an edge-major layout: log2 of its slots padded to a power of two (S), its iterations and the first of them in the
// flat stream.  False: some tile has more than 64 slots (`its` then counts the tiles before it).
struct EmCounts { std::vector<int32_t> it0, lgS, nit; int64_t its = 0; };
bool em_iteration_counts(const bt_plan *pl, EmCounts &c) {
    const int64_t T = pl->info.tiles;
    c.it0.assign((size_t)T, 0); c.lgS.assign((size_t)T, 0); c.nit.assign((size_t)T, 0);
    for (int64_t t = 0; t < T; ++t) {
        const int lg = ceil_log2(pl->tile_nslot[(size_t)t]);
        if (lg > 6) return false;
        c.it0[(size_t)t] = (int32_t)c.its; c.lgS[(size_t)t] = lg; c.nit[(size_t)t] = em_iterations(pl->tile_ntrk[(size_t)t], kLanes >> lg);
        c.its += c.nit[(size_t)t];
    }
    return true;
}
// ... into tile_rec[6], [7], and em_lgs
void em_record(bt_plan *pl, const EmCounts &c) {
    const int64_t T = pl->info.tiles;
    for (int64_t t = 0; t < T; ++t) {
        pl->tile_rec[(size_t)t * 8 + 6] = c.it0[(size_t)t];
        pl->tile_rec[(size_t)t * 8 + 7] = c.lgS[(size_t)t] | (c.nit[(size_t)t] << 8);
        if (t == 0) pl->dev.em_lgs = c.lgS[0]; else if (pl->dev.em_lgs != c.lgS[(size_t)t]) pl->dev.em_lgs = -1;
    }
}

// ---- edge-major layout of the same tiles (k_edge2 / k_edge2u, ba_edge2.hip / ba_edge2u.hip): the slots of a track padded to S = the next
// power of two, an ITERATION = 64 lanes = 64 / S consecutive tracks x S slots (lane = track_in_iteration * S + slot),
// so that on the caller's track-major edge lists a wave reads 64 consecutive edges, a track's sums are reductions over
// S adjacent lanes, and a lane meets the same camera pair in every iteration of a tile (per-lane pair sums, no
// wave-wide reduction per slot).  Usable when every tile is SLOT-UNIFORM: all tracks of the tile have the same pair
// (or no edge) in slot s.
//   it_edge[(it0 + i) * 64 + lane]   edge of (tile, iteration i, lane), -1 = none
//   tile_sinfo[t * 64 + s]           local target camera | local pair << 8 | repeat << 16 | used << 17   (s < S)
//                                    repeat: this slot or a neighbour holds the same pair again (repeated observation)
//   tile_rec[6] = it0, tile_rec[7] = log2 S | iterations << 8
int edge_major_tables(PlanBuild &b) {
    bt_plan *pl = b.pl;
    const bt_plan_info &I = pl->info;
    pl->dev.em_ok = 0; pl->dev.em_its = 0; pl->dev.em_lgs = -1;
    if (!(b.dev_wpt || b.want_stream_tables) || I.tiles < b.em_min_p) return BT_OK;
    EmCounts c;
    pl->dev.em_ok = em_iteration_counts(pl, c) ? 1 : 0;
    if (c.its > INT32_MAX) return BT_EUNSUPPORTED;               // (PlanDev::em_its is an int)
    if (b.dev_wpt) {
        // (the iteration counts follow from the tiles' slot and track counts; whether every tile is slot-uniform is k_plan_sinfo's
        //  verdict, read back by upload_plan: em_ok here is "as far as the host can tell")
        if (pl->dev.em_ok) em_record(pl, c);
        pl->dev.em_its = pl->dev.em_ok ? (int)c.its : 0;
        return BT_OK;
    }
    pl->tile_sinfo.assign(pl->dev.em_ok ? (size_t)I.tiles * kLanes : 0, 0);
    for (int64_t t = 0; t < I.tiles && pl->dev.em_ok; ++t) {
        const size_t b0 = (size_t)pl->tile_slot0[(size_t)t] * kLanes;
        const int32_t ns = pl->tile_nslot[(size_t)t], nt = pl->tile_ntrk[(size_t)t];
        for (int32_t sl = 0; sl < ns && pl->dev.em_ok; ++sl) {
            int32_t code = -1;
            for (int ln = 0; ln < nt; ++ln) {
                const size_t i = b0 + (size_t)sl * kLanes + (size_t)ln;
                if (pl->slot_edge[i] < 0) continue;
                const int32_t cd = (int32_t)pl->slot_code[i];
                if (code < 0) code = cd; else if (code != cd) { pl->dev.em_ok = 0; break; }
            }
            if (code >= 0) pl->tile_sinfo[(size_t)t * kLanes + (size_t)sl] = (uint32_t)code | (1u << 17);
        }
        for (int32_t sl = 0; sl + 1 < ns && pl->dev.em_ok; ++sl) {
            uint32_t &x = pl->tile_sinfo[(size_t)t * kLanes + (size_t)sl], &y = pl->tile_sinfo[(size_t)t * kLanes + (size_t)sl + 1];
            if ((x >> 17 & 1u) && (y >> 17 & 1u) && ((x >> 8) & 0xffu) == ((y >> 8) & 0xffu)) { x |= 1u << 16; y |= 1u << 16; }
        }
    }
    if (pl->dev.em_ok) {
        pl->it_edge.assign((size_t)c.its * kLanes, -1);
        for (int64_t t = 0; t < I.tiles; ++t) {
            const size_t b0 = (size_t)pl->tile_slot0[(size_t)t] * kLanes;
            const int32_t ns = pl->tile_nslot[(size_t)t], nt = pl->tile_ntrk[(size_t)t], lg = c.lgS[(size_t)t], G = kLanes >> lg;
            for (int32_t k = 0; k < nt; ++k)
                for (int32_t sl = 0; sl < ns; ++sl)
                    pl->it_edge[((size_t)c.it0[(size_t)t] + (size_t)(k / G)) * kLanes + (size_t)((k % G) << lg) + (size_t)sl] =
                        pl->slot_edge[b0 + (size_t)sl * kLanes + (size_t)k];
        }
        em_record(pl, c);
    } else {
        pl->it_edge.clear(); pl->tile_sinfo.clear();
    }
    pl->dev.em_its = pl->dev.em_ok ? (int)c.its : 0;
    return BT_OK;
}

// the pair-major tables from the [slots][64] arrays of 64-track tiles (pair_major_tables)
void pair_major_from_slots(PlanBuild &b, int pm_env) {
    bt_plan *pl = b.pl;
    const bt_plan_info &I = pl->info;
    pl->pm_rec.assign((size_t)I.tiles * 4, 0);
    pl->pm_lb.assign((size_t)I.tiles * kLanes, 0xff);
    pl->pm_la.assign((size_t)I.tiles * kLanes, 0xff);
    std::vector<int32_t> cnt;                              // edges of (track, local pair) placed so far
    int64_t rounds = 0;
    for (int64_t t = 0; t < I.tiles && pl->dev.pm_ok; ++t) {
        const size_t b0 = (size_t)pl->tile_slot0[(size_t)t] * kLanes;
        const int32_t ns = pl->tile_nslot[(size_t)t], nt = pl->tile_ntrk[(size_t)t], np = pl->tile_npair[(size_t)t];
        const int lg = ceil_log2(np);
        const int32_t S = 1 << lg, G = kLanes >> lg, nit = (nt + G - 1) / G;
        // multiplicities
        cnt.assign((size_t)nt * (size_t)S, 0);
        int32_t D = 1;
        for (int32_t k = 0; k < nt; ++k)
            for (int32_t sl = 0; sl < ns; ++sl) {
                const size_t i = b0 + (size_t)sl * kLanes + (size_t)k;
                if (pl->slot_edge[i] < 0) continue;
                D = std::max(D, ++cnt[(size_t)k * S + pl->slot_lp[i]]);
            }
        if (D > 255) { pl->dev.pm_ok = 0; break; }
        pl->pm_rec[(size_t)t * 4] = (int32_t)rounds;
        pl->pm_rec[(size_t)t * 4 + 1] = lg | (D << 8);
        pl->pm_rec[(size_t)t * 4 + 2] = nit;
        pl->pm_edge.resize((size_t)(rounds + (int64_t)nit * D) * kLanes, -1);
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int32_t k = 0; k < nt; ++k)
            for (int32_t sl = 0; sl < ns; ++sl) {
                const size_t i = b0 + (size_t)sl * kLanes + (size_t)k;
                if (pl->slot_edge[i] < 0) continue;
                const int32_t lp = pl->slot_lp[i], d = cnt[(size_t)k * S + lp]++;
                pl->pm_edge[pm_index(rounds, k, G, D, d, lg, lp)] = pl->slot_edge[i];
                pl->pm_lb[(size_t)t * kLanes + (size_t)lp] = (uint8_t)(pl->slot_lab[i] >> 8);
                pl->pm_la[(size_t)t * kLanes + (size_t)k] = (uint8_t)(pl->slot_lab[i] & 0xff);
            }
        rounds += (int64_t)nit * D;
    }
    pl->pm_rounds = rounds;
    if (pl->dev.pm_ok && (b.tcap < kLanes || pm_env == 2)) pl->dev.pm_ok = 2;
    if (!pl->dev.pm_ok) clear_pair_major(pl);
}

// ---- pair-major layout of the same tiles (k_etile, ba_etile.hip): lane = track_in_iteration * S + s, where s is the LOCAL
// PAIR of the tile (S = its pair count padded to a power of two, an iteration = 64 / S consecutive tracks) and the edges a
// track has with that pair — repeated observations (batrack.py:399-410 appends a window's factors again every keyframe
// step) — are the lane's D ROUNDS.  A lane then keeps one camera pair for the whole tile (the 27 per-pair products are
// summed per lane in registers), owns its (track, target camera) element of the local E exclusively (plain store of the
// sum over its rounds), and a track's own sums (C, w, source-camera E) are reductions over S adjacent lanes.  Any tile of
// at most 64 pairs can be laid out this way (a track that lacks a pair has no edge in that lane).
//   pm_edge[(round0 + it * D + d) * 64 + lane]   edge of (tile, iteration it, round d, lane), -1 = none
//   pm_rec[t * 4]   = round0, log2 S | D << 8, iterations, 0
//   pm_lb[t * 64 + s]   local target camera of local pair s (0xff: fixed, or s >= npair)
//   pm_la[t * 64 + l]   local source camera of track l of the tile (0xff: fixed / no track)
// pm_ok: 2 = the plan was tiled FOR the pair-major kernel (small tiles) or BT_ETILE=2 forces it, 1 = the tables exist but
// k_tile keeps the plan (at one tile per CU, e.g. the 64-keyframe benchmark, k_tile measured 12.7 us against 15.0)
int pair_major_tables(PlanBuild &b) {
    bt_plan *pl = b.pl;
    const bt_plan_info &I = pl->info;
    const bool etile_fits = etile_full_lds_bytes(pl->dev.max_rows16, pl->dev.max_tile_pairs, sizeof(double)) <= kEtileLdsBudget;
    pl->dev.pm_ok = I.tiles > 0 ? 1 : 0; pl->pm_rounds = 0;
    if (b.dstats) {
        if (I.tiles <= 0) return BT_NEED_EDGES;
        if (b.pm_direct) {
            // small tiles are for k_etile only: lay the plan out again for k_tile
            if (b.pm_fail || !etile_fits) return b.lay.small_tiles_allowed ? (int)kRelayoutLargeTiles : (int)BT_NEED_EDGES;
            pl->dev.pm_ok = 2; pl->dev_pm = 1;
        } else {
            pl->dev.pm_ok = 0; pl->dev_slots = 1;
            clear_pair_major(pl);
            pl->dev_off = b.off;
        }
        pl->dev_pair_of = b.pair_of; pl->dev_f_lo = b.f_lo; pl->dev_nw = b.nw;
    } else if (b.pm_direct) {
        // (built tile by tile, pair_major_tile) — the plan stays with k_etile only if that kernel's LDS need fits in float64
        if (b.pm_fail || I.tiles <= 0 || !etile_fits) {
            pl->dev.pm_ok = 0;
            clear_pair_major(pl);
        } else {
            pl->dev.pm_ok = 2;
            pl->pm_rounds = b.pm_rounds_acc;
        }
    } else {
        clear_pair_major(pl);
    }
    if (!b.pm_direct) {
        const int pm_env = etile_mode();                            // 0: k_tile forced
        if (!pm_env || (pm_env != 2 && b.tcap == kLanes)) pl->dev.pm_ok = 0;      // (tables only for the plans that will use them)
        if (!b.loose.empty()) pl->dev.pm_ok = 0;                                   // (k_etile's stored per-tile sums bypass the accumulators the loose tracks add to)
        for (int64_t t = 0; t < I.tiles && pl->dev.pm_ok; ++t) if (pl->tile_npair[(size_t)t] > kLanes) pl->dev.pm_ok = 0;
        if (pl->dev.pm_ok) pair_major_from_slots(b, pm_env);
    }
    // small tiles are for k_etile only: lay the plan out again for k_tile
    // (a device-planned list does not come here: its small tiles either asked for this above or have pm_ok = 2)
    if (!pl->dev.pm_ok && b.tcap < kLanes && b.lay.small_tiles_allowed) return kRelayoutLargeTiles;
    return BT_OK;
}

// ---- partial sums instead of atomics for the pair-major kernel: hundreds of workgroups' float64 atomics on the same few
// thousand elements of [S | y] and of the per-pair sums queue up in the L2 (measured on the 160-tile window: half of the
// kernel).  Every tile stores its Schur product, E Q w' and pair sums (StepArgs::spart); k_pair_finalize adds them up —
// the products by position over each GROUP of consecutive tiles with the same cameras (a sliding window: the tiles of one
// source frame; at most kSpGroupMax tiles, so that the sum is one round of independent loads), the pair sums over the
// plan's list of every pair's (tile, local pair) entries.
void partial_sum_tables(bt_plan *pl) {
    const bt_plan_info &I = pl->info;
    pl->dev.sp_ok = 0;
    int mt = 1;
    for (int64_t t = 0; t < I.tiles; ++t) mt = std::max(mt, (int)pl->tile_ntrk[(size_t)t]);
    pl->dev.et_lgts = ceil_log2(mt);
    if (pl->dev.pm_ok == 2 && ((int64_t)sp_tile_doubles(pl->dev.max_rows16, pl->dev.max_tile_pairs) + ((int64_t)pl->dev.max_rows16 << pl->dev.et_lgts)) * I.tiles * 8 <= ((int64_t)96 << 20)) pl->dev.sp_ok = 1;
    pl->sg_ptr.clear();
    pl->pp_ptr.clear(); pl->pp_idx.clear();
    if (!pl->dev.sp_ok) return;
    for (int64_t t = 0; t < I.tiles; ++t)
        if (t == 0 || !(pl->tile_flags[(size_t)t] & 1) || t - pl->sg_ptr.back() >= kSpGroupMax) pl->sg_ptr.push_back((int32_t)t);
    pl->sg_ptr.push_back((int32_t)I.tiles);
    // which tiles hold sums of which camera pair
    pl->pp_ptr.assign((size_t)I.pairs + 1, 0);
    for (size_t q = 0; q < pl->tile_pairs.size(); ++q) pl->pp_ptr[(size_t)pl->tile_pairs[q] + 1]++;
    for (int64_t p = 0; p < I.pairs; ++p) pl->pp_ptr[(size_t)p + 1] += pl->pp_ptr[(size_t)p];
    pl->pp_idx.assign(pl->tile_pairs.size(), 0);
    std::vector<int32_t> cur(pl->pp_ptr.begin(), pl->pp_ptr.end() - 1);
    for (int64_t t = 0; t < I.tiles; ++t)
        for (int32_t q = 0; q < pl->tile_npair[(size_t)t]; ++q)
            pl->pp_idx[(size_t)cur[(size_t)pl->tile_pairs[(size_t)(pl->tile_pair0[(size_t)t] + q)]]++] = (int32_t)(t << 6) | q;
}

// ---- k_update: which patches carry a track (bitmap + rank per 32 patches: the patch buffer is BUFFER_SIZE x M
// = 262,144 slots in the reference's configuration, the window's tracks a few thousand)
void activity_bitmap(bt_plan *pl) {
    const size_t nwords = (size_t)((pl->info.p_tot + 31) / 32);
    pl->act_bits.assign(nwords, 0u);
    pl->act_rank.assign(nwords, 0);
    for (int32_t k = 0; k < pl->info.m; ++k) pl->act_bits[(size_t)(pl->kx[(size_t)k] >> 5)] |= 1u << (pl->kx[(size_t)k] & 31);
    int32_t run = 0;
    for (size_t w = 0; w < nwords; ++w) { pl->act_rank[w] = run; run += __builtin_popcount(pl->act_bits[w]); }
}

// One layout attempt: everything from the tiling on.  BT_OK, an error, or a kRelayout... request.
int lay_out(PlanBuild &b, const Layout &lay) {
    bt_plan *pl = b.pl;
    bt_plan_info &I = pl->info;
    I = b.info0;
    pl->dev_pm = 0; pl->dev_slots = 0; pl->dev_wpt = 0;
    b.lay = lay;
    b.loose.clear(); b.tile_tmask.clear();
    b.slots = 0; b.erows = 0; b.max_cams = 0;
    pl->tile_trk0.clear(); pl->tile_ntrk.clear(); pl->tile_ncam.clear(); pl->tile_cam0.clear();
    pl->tile_slot0.clear(); pl->tile_nslot.clear(); pl->tile_erow0.clear(); pl->tile_cams.clear();
    pl->trk_loc.assign((size_t)b.m, 0);
    pl->dev_pbase.clear();
    int rc = choose_layout(b);
    if (rc != BT_OK) return rc;
    Tiler tl;
    rc = b.aligned ? tile_tracks_aligned(b, tl) : tile_tracks(b, tl);
    if (rc != BT_OK) return rc;
    // (many long tracks: tiles of up to 64 cameras, float32 per edge)
    if (lay.cam_hard != kTileCamHard && (int)b.loose.size() > kFewHubs) return kRelayoutHubsInTiles;
    const int32_t T = (int32_t)pl->tile_trk0.size();
    I.tiles = T; I.slots = b.slots; I.erows = b.erows; I.max_tile_cams = b.max_cams;
    pl->dev.max_rows16 = (int)((6 * b.max_cams + 15) / 16 * 16);
    if (b.tcap < kLanes && T >= std::min(std::min(b.em_min_p, b.st_min_p), 1024)) {
        // the camera limit closed 16-track tiles early: the plan reached the tile count of the wave-per-tile kernels, whose
        // tables come from the [slots][64] arrays a small-tile plan does not have — or simply four times the CUs, where
        // spreading a graph over more workgroups has lost its point: lay it out again with 64 tracks per tile
        return lay.small_tiles_allowed ? (int)kRelayoutLargeTiles : b.dstats ? (int)BT_NEED_EDGES : (int)BT_EUNSUPPORTED;
    }

    b.tick("6");
    if ((rc = fill_tiles(b)) != BT_OK) return rc;
    loose_lists_and_tile_flags(b);

    b.tick("8");
    if ((rc = plan_reduced_system(pl, b.sharded, b.dstats, b.pk, b.E, b.tick)) != BT_OK) return rc;

    b.tick("13");
    tile_first_loads(pl);
    stream_tables(b);
    if ((rc = edge_major_tables(b)) != BT_OK) return rc;
    if ((rc = pair_major_tables(b)) != BT_OK) return rc;
    partial_sum_tables(pl);

    b.tick("14");
    pl->dev.max_tile_slots = 0;
    for (int64_t t = 0; t < I.tiles; ++t) pl->dev.max_tile_slots = std::max(pl->dev.max_tile_slots, (int)pl->tile_nslot[(size_t)t]);
    activity_bitmap(pl);

    b.tick("end");
    layout_workspace(pl);
    return BT_OK;
}

}  // namespace

int build_plan_host(const int64_t *ii64, const int64_t *jj64, const int64_t *kk64, int64_t E,
                    int64_t n_buf, int64_t p_tot, int64_t fixedp, int64_t n_all_min,
                    int64_t own_lo, int64_t own_hi, bt_plan *pl, const uint64_t *packed, bool keep_slots, const DevPlanStats *dstats) {
    if (E < 0 || n_buf <= 0 || p_tot <= 0 || fixedp < 0 || n_all_min < 0 || n_all_min > n_buf) return BT_EINVAL;
    if (E > (int64_t)0x7fffffff / 2 || p_tot > (int64_t)0x7fffffff) return BT_EUNSUPPORTED;
    if (n_buf > 32768) return BT_EUNSUPPORTED;             // frame numbers are packed in pairs into signed 32-bit words (tile_ij)
    bt_plan_info &I = pl->info;
    I = bt_plan_info{};
    I.n_buf = n_buf; I.p_tot = p_tot; I.fixedp = fixedp;
    pl->dev.e_all = E;
    PlanScratch &s = scratch();
    PlanBuild b(s);
    // A plan of a SHARDED solve (the caller named a track range, whatever it covers): the ranks exchange [S | y] block by block of the
    // factor's pattern, so every rank must arrive at the same pattern — from what all of them can see, the tracks of the whole list.
    b.sharded = own_hi > 0;
    if (own_hi <= 0) { own_lo = 0; own_hi = p_tot; }
    if (own_lo < 0 || own_hi > p_tot || own_lo > own_hi) return BT_EINVAL;
    b.E = E; b.n_buf = n_buf; b.p_tot = p_tot; b.fixedp = fixedp; b.own_lo = own_lo; b.own_hi = own_hi;
    b.pk = packed; b.dstats = dstats; b.keep_slots = keep_slots; b.pl = pl;

    b.tick("0");
    pl->dev_pm = 0; pl->dev_slots = 0; pl->dev_wpt = 0;
    if (dstats && (keep_slots || E <= 0)) return BT_NEED_EDGES;
    if (!b.pk && !dstats) {
        s.pk.resize((size_t)E + 1);
        const int rc = pack_edges_host(ii64, jj64, kk64, E, n_buf, p_tot, s.pk.data());
        if (rc != BT_OK) return rc;
        b.pk = s.pk.data();
    }
    s.rep_host.clear();
    if ((int64_t)s.pp_tab.size() < p_tot) { s.pp_tab.assign((size_t)p_tot, PerPatch{0, 0, 0, 0, 0, 0}); s.pp_lo = 0; s.pp_hi = -1; }
    for (int64_t p = s.pp_lo; p <= s.pp_hi; ++p) s.pp_tab[(size_t)p].cnt = 0;
    b.pp = s.pp_tab.data();
    b.n_all = n_all_min; b.kmin = p_tot; b.kmax = -1; b.f_lo = n_buf;
    b.cj.assign((size_t)n_buf + 2, 0);
    if (dstats) { if (scan_device_table(b) != BT_OK) return BT_NEED_EDGES; }
    else scan_edges(b);
    s.pp_lo = b.kmin; s.pp_hi = b.kmax;
    int rc = edge_pass_figures(b);
    if (rc != BT_OK) return rc;

    b.tick("1");
    number_tracks(b);
    b.tick("2");
    number_pairs(b);
    b.tick("3");
    group_edges(b);
    b.tick("4");

    // The layout: again from the tiling with one knob changed for as long as a phase asks for it.  Each knob moves once and a
    // phase asks only for one that has not moved, so this ends after at most four attempts.
    b.info0 = I;
    Layout lay;
    for (;;) {
        rc = lay_out(b, lay);
        if (rc == kRelayoutLargeTiles) lay.small_tiles_allowed = false;
        else if (rc == kRelayoutUnaligned) lay.aligned_allowed = false;
        else if (rc == kRelayoutHubsInTiles) lay.cam_hard = kTileCamHard;
        else return rc;
        // A plan that is laid out again takes the pattern of S from its tracks' own couplings, as a sharded plan does, whether
        // the caller named a range or not: the recursion this loop replaces handed its defaulted range [0, p_tot) on, which
        // reads as one.  Kept as it is — the pattern decides the solver's tables, and theirs is the smaller one, as valid as
        // the tiles' (ba_plan_solver.cpp: system_pattern).
        b.sharded = true;
    }
}

}  // namespace bt
