// ba_api.cpp — the C ABI declared in include/batrack_ba.h.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <utility>

#include "plan_host.hpp"

#define BT_VERSION 204

namespace bt {

template <class T>
static size_t put(std::vector<char> &buf, const std::vector<T> &v) {
    size_t off = (buf.size() + 255) / 256 * 256;
    buf.resize(off + v.size() * sizeof(T) + 1);
    if (!v.empty()) std::memcpy(buf.data() + off, v.data(), v.size() * sizeof(T));
    return off;
}

DevPool &dev_pool() { static DevPool *p = new DevPool(); return *p; }   // never destroyed: no HIP call at exit

PlanPool &plan_pool() { static PlanPool *p = new PlanPool(); return *p; }

// Plan transfers (index download, table upload) run on a stream of their own, created non-blocking: a plan can
// then be built from a second host thread while the caller's streams are busy — BATRACK knows the edge list of an
// update() a whole tracker pass before it calls the BA (batrack.py:983-993) — without the implicit waits a
// synchronous hipMemcpy on the null stream would bring.
hipStream_t copy_stream() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    static std::mutex mu;
    static std::vector<std::pair<int, hipStream_t>> *streams = new std::vector<std::pair<int, hipStream_t>>();
    std::lock_guard<std::mutex> lk(mu);
    for (auto &e : *streams) if (e.first == dev) return e.second;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;   // null stream: still correct
    streams->emplace_back(dev, s);
    return s;
}

PackBuffers &pack_buffers() { static thread_local PackBuffers pb; return pb; }

void bind_pointers(bt_plan *pl, const void *d) {
    const char *b = static_cast<const char *>(d);
    const bt_plan_info &I = pl->info;
    PlanDev &P = pl->dev;
    P.E = (int)I.E; P.n_buf = (int)I.n_buf; P.p_tot = (int)I.p_tot; P.fixedp = (int)I.fixedp;
    P.n_all = (int)I.n_all; P.n = (int)I.n; P.D = (int)(6 * I.n); P.m = (int)I.m; P.P = (int)I.pairs;
    P.T = (int)I.tiles; P.slots = (int)I.slots; P.erows = (int)I.erows; P.nnzb = (int)I.nnz_blocks;
    P.nupd = (int)I.updates; P.max_cams = (int)I.max_tile_cams;
#define BT_BIND(T, name, solver) P.name = reinterpret_cast<const T *>(b + pl->off[tab::name]);
    BT_PLAN_TABLES(BT_BIND)
#undef BT_BIND
}

// Plans of up to this many edges keep their packed edge list on the device (8 bytes per edge) so that the next edge
// list can be recognised as a shifted copy (bt_plan_create_shifted)
constexpr int64_t kKeepPackedMaxEdges = 4 << 20;

int upload_plan(bt_plan *pl, const uint64_t *d_packed) {
    PhaseTimer tick{"plan api"};
    std::vector<char> &buf = pl->stage;           // capacity survives with the recycled plan object
    buf.clear();
#define BT_PUT(T, name, solver) pl->off[tab::name] = put(buf, pl->name); pl->len[tab::name] = pl->name.size();
    BT_PLAN_TABLES(BT_PUT)
#undef BT_PUT
    PlanDev &P = pl->dev;
    P.nlev = (int)pl->lvl_ptr.size() - 1; P.ndp = (int)pl->dp.size();
    P.fz_npend = (int)(pl->fz_pend.size() / 2); P.fz_nlazy = (int)(pl->fz_lazy.size() / 3);
    P.nlz = (int)pl->lz_trk.size();
    P.sg_n = pl->sg_ptr.empty() ? 0 : (int)pl->sg_ptr.size() - 1;
    tick("pack arrays");
    const bool keep_pk = d_packed && P.e_all > 0 && P.e_all <= kKeepPackedMaxEdges && pl->info.E == P.e_all;
    // (tables the device writes lie behind the staged bytes, nothing of them crosses PCIe: pm_edge of a plan whose pair-major
    //  table is written there, the [slots][64] arrays of a 64-track layout and with them the tables of the wave-per-tile kernels)
    size_t tables_end = buf.size();
    auto take = [&](int t, size_t n, size_t esz) { pl->off[t] = (tables_end + 255) / 256 * 256; pl->len[t] = n; tables_end = pl->off[t] + n * esz; };
    if (pl->dev_pm) take(tab::pm_edge, (size_t)pl->pm_rounds * kLanes, sizeof(int32_t));
    if (pl->dev_slots) {
        const size_t ns = (size_t)pl->info.slots * kLanes, tl = (size_t)pl->info.tiles * kLanes;
        take(tab::slot_edge, ns, sizeof(int32_t)); take(tab::slot_pair, ns, sizeof(int32_t)); take(tab::slot_lab, ns, sizeof(uint16_t)); take(tab::slot_lp, ns, 1);
        if (pl->dev_wpt) {
            take(tab::slot_code, ns, sizeof(uint16_t)); take(tab::tile_la, tl, 1);
            if (P.em_ok) { take(tab::it_edge, (size_t)P.em_its * kLanes, sizeof(int32_t)); take(tab::tile_sinfo, tl, sizeof(uint32_t)); }
        }
    }
    const size_t pk_off = (tables_end + 255) / 256 * 256, total = keep_pk ? pk_off + (size_t)P.e_all * sizeof(uint64_t) : tables_end;
    hipStream_t cs = copy_stream();
    size_t cap = 0;
    void *d = dev_pool().acquire(total + 256, cs, &cap);
    if (!d) return BT_ENOMEM;
    if (hipGetDevice(&P.dev_id) != hipSuccess) P.dev_id = 0;          // (once per plan: its launches take their per-device figures from it)
    bind_pointers(pl, d);                                  // (the fill kernels below read the plan's tile tables in the buffer)
    tick("device buffer");
    bool ok = hipMemcpyAsync(d, buf.data(), buf.size(), hipMemcpyHostToDevice, cs) == hipSuccess &&
              (!keep_pk || hipMemcpyAsync(static_cast<char *>(d) + pk_off, d_packed, (size_t)P.e_all * sizeof(uint64_t), hipMemcpyDeviceToDevice, cs) == hipSuccess);
    if (ok && (pl->dev_pm || pl->dev_slots)) {
        char *db = static_cast<char *>(d);
        auto at = [&](int t) { return db + pl->off[t]; };
        if (pl->dev_pm)
            ok = plan_device_fill(pl, pl->info.E, reinterpret_cast<int32_t *>(at(tab::pm_rec)), reinterpret_cast<int32_t *>(at(tab::pm_edge)), pl->pm_rounds, cs) == BT_OK;
        else {
            DevWptOut w{};
            if (pl->dev_wpt) {
                w.slot_code = reinterpret_cast<uint16_t *>(at(tab::slot_code)); w.tile_la = reinterpret_cast<uint8_t *>(at(tab::tile_la));
                w.tile_rec = reinterpret_cast<int32_t *>(at(tab::tile_rec));
                if (P.em_ok) { w.it_edge = reinterpret_cast<int32_t *>(at(tab::it_edge)); w.tile_sinfo = reinterpret_cast<uint32_t *>(at(tab::tile_sinfo)); w.its = P.em_its; }
            }
            ok = plan_device_slots_fill(pl, pl->info.E, reinterpret_cast<int32_t *>(at(tab::slot_edge)), reinterpret_cast<int32_t *>(at(tab::slot_pair)),
                                        reinterpret_cast<uint16_t *>(at(tab::slot_lab)), reinterpret_cast<uint8_t *>(at(tab::slot_lp)),
                                        reinterpret_cast<uint16_t *>(at(tab::tile_cut8)), reinterpret_cast<uint16_t *>(at(tab::tile_cut16)), cs,
                                        pl->dev_wpt ? &w : nullptr) == BT_OK;
        }
    }
    if (!ok || hipStreamSynchronize(cs) != hipSuccess) { dev_pool().release(d, cap, false, nullptr); return BT_EHIP; }
    // (k_plan_sinfo's verdict: a tile whose tracks do not share their slots' pairs leaves the plan with k_stream)
    if (pl->dev_slots && pl->dev_wpt && P.em_ok && plan_device_em_verdict()) { P.em_ok = 0; P.em_its = 0; P.em_lgs = -1; }
    tick("H2D copy");
    pl->dev_base = d;
    pl->dev_cap = cap;
    pl->dev_bytes = total;
    pl->pk_off = keep_pk ? pk_off : 0;
    const int rc = configure_kernels(P);
    tick("configure kernels");
    return rc;
}

static StepArgs make_args(const bt_plan *pl, const bt_ba_args *a, void *ws) {
    char *w = static_cast<char *>(ws);
    const WsLayout &L = pl->ws;
    StepArgs s{};
    s.poses = a->poses; s.patches = a->patches; s.mono = a->mono_disp; s.intr = a->intrinsics;
    s.targets = a->targets; s.weights = a->weights; s.tstride = (int)a->target_stride; s.mstride = a->mono_stride > 1 ? (int)a->mono_stride : 1;
    s.poses_out = a->poses_out; s.patches_out = a->patches_out;
    s.b0 = a->bounds[0]; s.b1 = a->bounds[1]; s.b2 = a->bounds[2]; s.b3 = a->bounds[3];
    s.lmbda = a->lmbda; s.ep = a->ep; s.alpha = a->alpha; s.loss = a->loss;
    s.lmbda_trk = a->lmbda_per_track;
    const size_t D = (size_t)(6 * pl->info.n);
    s.S = reinterpret_cast<double *>(w + L.sys); s.y = s.S + D * D;
    s.pairacc = reinterpret_cast<double *>(w + L.pairacc);
    // (k_edge2's private copies: only where k_edge2 is the plan's Jacobian kernel — k_pair_finalize adds up what it is given)
    s.priv = L.priv && pl->dev.route.kernel == Route::kEdge ? reinterpret_cast<double *>(w + L.priv) : nullptr;
    s.pairgeo = reinterpret_cast<float *>(w + L.pairgeo);
    s.packed = reinterpret_cast<double *>(w + L.packed); s.qw = reinterpret_cast<float2 *>(w + L.qw);
    s.lfac = reinterpret_cast<float *>(w + L.lfac);
    s.linv = reinterpret_cast<float *>(w + L.linv); s.zvec = reinterpret_cast<float *>(w + L.zvec);
    s.dx = reinterpret_cast<float *>(w + L.dx); s.dx0 = reinterpret_cast<float *>(w + L.dx0);
    s.dxg = reinterpret_cast<unsigned long long *>(w + L.dxg); s.status = reinterpret_cast<int *>(w + L.status);
    s.spart = reinterpret_cast<double *>(w + L.spart);
    s.esave = reinterpret_cast<double *>(w + L.esave);
    static const int dbg = std::getenv("BT_DEBUG_MODE") ? std::atoi(std::getenv("BT_DEBUG_MODE")) : 0;
    s.dbg = dbg;
    s.prec = pl->dev.route.prec == 8 ? 1 : 0;
    return s;
}

// Every entry point that launches a plan's kernels passes here first: the stream is remembered for bt_plan_destroy, and a clone
// whose tables are still being copied on the plan stream (plan_shift.cpp: clone_shifted) gets its launches ordered behind them.
static void mark_launch(const bt_plan *pl, void *stream) {
    pl->last_stream = stream; pl->launched = true;
    if (void *r = pl->ready.load(std::memory_order_acquire)) {
        hipEvent_t ev = static_cast<hipEvent_t>(r);
        if (hipEventQuery(ev) == hipSuccess) {
            if (pl->ready.exchange(nullptr, std::memory_order_acq_rel) == r) dev_pool().give_event(ev);      // (one claimant)
        }
        else if (hipStreamWaitEvent(static_cast<hipStream_t>(stream), ev, 0) != hipSuccess) (void)hipEventSynchronize(ev);
    }
}

static int check(const bt_plan *pl, const bt_ba_args *a, const void *ws) {
    if (!pl || !a || !ws || !pl->dev_base) return BT_EINVAL;
    if (pl->spec.state == SpecState::kUnbound) return BT_EINVAL;                 // (a clone made ahead of its list, never given it: bt_plan_spec_bind)
    if (!a->poses || !a->patches || !a->mono_disp || !a->intrinsics || !a->patches_out) return BT_EINVAL;
    if (pl->info.E > 0 && (!a->targets || !a->weights || a->target_stride < 2)) return BT_EINVAL;
    if (a->loss < BT_LOSS_TRIVIAL || a->loss > BT_LOSS_CAUCHY) return BT_EINVAL;
    if (a->mono_stride < 0) return BT_EINVAL;                 // 0 and 1 both mean contiguous; a prior of one repeated element must be materialised
    return BT_OK;
}

// ba.py:316: "structure_only or n == 0" take the same branch
static bool is_so(const bt_plan *pl, const bt_ba_args *a) { return a->structure_only != 0 || pl->info.n == 0; }

// What the entry points that run a step's solve / update half validate before anything is enqueued: check(), and that poses_out
// is there and distinct from poses — unless the step is structure-only, which copies the poses where it is given such a poses_out
struct StepMode { int rc; bool so, copy_poses; };
static StepMode step_mode(const bt_plan *pl, const bt_ba_args *a, const void *ws) {
    StepMode m{check(pl, a, ws), false, false};
    if (m.rc != BT_OK) return m;
    m.so = is_so(pl, a);
    const bool distinct = a->poses_out && a->poses_out != a->poses;
    if (!m.so && !distinct) m.rc = BT_EINVAL;
    m.copy_poses = m.so && distinct;
    return m;
}

}  // namespace bt

using namespace bt;

extern "C" {

int bt_version(void) { return BT_VERSION; }
int bt_plan_jacobian_kernel(const bt_plan *pl) {
    if (!pl || !pl->dev_base) return -1;
    return pl->dev.route.kernel;
}
int bt_plan_built_on_device(const bt_plan *pl) { return pl && (pl->dev_pm || pl->dev_slots) ? 1 : 0; }

int bt_plan_edge_precision(const bt_plan *pl) {
    if (!pl || !pl->dev_base) return -1;
    return pl->dev.route.prec;                      // 6: mixed (ba_edge.hpp: edge_eval_mixed)
}
const char *bt_target_arch(void) { return "gfx950"; }

int bt_plan_create(const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E, int64_t n_buf,
                   int64_t p_tot, int64_t fixedp, int64_t n_all_min, int64_t own_lo, int64_t own_hi,
                   int on_device, int upload, bt_plan **out) {
    if (!out || E < 0 || (E > 0 && (!ii || !jj || !kk))) return BT_EINVAL;
    *out = nullptr;
    const uint64_t *packed = nullptr;
    PhaseTimer tick{"plan api"};
    if (on_device && E > 0) {
        // packed and range-checked on the device (8 of the 24 bytes per edge cross PCIe), into a pinned host buffer
        if (!buffers_packable(n_buf, p_tot)) return BT_EUNSUPPORTED;
        PackBuffers &pb = pack_buffers();
        if (!pb.ensure((size_t)E)) return BT_ENOMEM;
        hipStream_t cs = copy_stream();
        if (hipMemsetAsync(pb.d_bad, 0, sizeof(int), cs) != hipSuccess ||
            launch_pack_edges(ii, jj, kk, E, n_buf, p_tot, pb.d_words, pb.d_bad, cs) != BT_OK)
            return BT_EHIP;
        // window plans: the passes over the edges stay on the device (plan_device.hip), the host lays out what is small
        const bool dev_planner = !force().host_plan;
        if (dev_planner && upload && E >= 4096) {
            if (hipMemcpyAsync(pb.h_bad, pb.d_bad, sizeof(int), hipMemcpyDeviceToHost, cs) != hipSuccess) return BT_EHIP;
            DevPlanStats st{};
            int64_t tracks = 0;
            int rc = plan_device_stats(pb.d_words, E, p_tot, fixedp, own_lo, own_hi, cs, &st, &tracks);       // (rc == BT_OK: it synchronised, h_bad is in as well)
            if (rc != BT_OK && rc != BT_NEED_EDGES) return rc;
            // (BT_NEED_EDGES can come back before anything was waited for — p_tot or E beyond the device path — and h_bad may
            //  then still hold an earlier list's verdict: it is read only behind a synchronisation; the host path below does its own)
            if (rc == BT_OK && *pb.h_bad) return BT_EINVAL;
            tick("device: per-track figures");
            if (rc == BT_OK) {
                bt_plan *pl = plan_pool().take();
                if (!pl) return BT_ENOMEM;
                try {
                    rc = build_plan_host(nullptr, nullptr, nullptr, E, n_buf, p_tot, fixedp, n_all_min, own_lo, own_hi, pl, nullptr, false, &st);
                    tick("host analysis (no edges)");
                    int64_t rounds = 0;
                    if (rc == BT_OK) rc = pl->dev_pm ? plan_device_rounds(pl, pl->info.E, cs, &rounds) : plan_device_slots_stage(pl, cs);
                    tick("device: rounds");
                    if (rc == BT_OK) { pl->pm_rounds = rounds; rc = upload_plan(pl, pb.d_words); }
                } catch (const std::bad_alloc &) {
                    rc = BT_ENOMEM;
                }
                if (rc == BT_OK) { *out = pl; return BT_OK; }
                bt_plan_destroy(pl);
                if (rc != BT_NEED_EDGES) return rc;
            }
        }
        if (hipMemcpyAsync(pb.h_words, pb.d_words, (size_t)E * sizeof(uint64_t), hipMemcpyDeviceToHost, cs) != hipSuccess ||
            hipMemcpyAsync(pb.h_bad, pb.d_bad, sizeof(int), hipMemcpyDeviceToHost, cs) != hipSuccess ||
            hipStreamSynchronize(cs) != hipSuccess)
            return BT_EHIP;
        if (*pb.h_bad) return BT_EINVAL;
        packed = pb.h_words;
        tick("D2H indices");
    }
    bt_plan *pl = plan_pool().take();
    if (!pl) return BT_ENOMEM;
    int rc = BT_OK;
    try {
        rc = build_plan_host(packed ? nullptr : ii, packed ? nullptr : jj, packed ? nullptr : kk, E, n_buf, p_tot, fixedp, n_all_min, own_lo, own_hi, pl, packed, /*keep_slots=*/!upload);
        tick("host analysis");
        if (rc == BT_OK && upload) rc = upload_plan(pl, packed ? pack_buffers().d_words : nullptr);
    } catch (const std::bad_alloc &) {
        rc = BT_ENOMEM;
    }
    if (rc != BT_OK) { bt_plan_destroy(pl); return rc; }
    *out = pl;
    return BT_OK;
}

void bt_plan_destroy(bt_plan *pl) {
    if (!pl) return;
    // an unsettled speculation, by state (the fields themselves go with recycle())
    if (pl->spec.state == SpecState::kEvent) { (void)hipEventSynchronize(static_cast<hipEvent_t>(pl->spec.event)); dev_pool().give_event(static_cast<hipEvent_t>(pl->spec.event)); }
    if (pl->spec.state == SpecState::kPolled) (void)hipStreamSynchronize(static_cast<hipStream_t>(pl->spec.stream));   // (a comparison that reads this plan's words may still be queued)
    if (void *r = pl->ready.exchange(nullptr, std::memory_order_acq_rel)) {
        // (copies of a clone that was never launched may still be queued on the plan stream: the buffer's next owner writes it
        //  on that same stream, behind them)
        dev_pool().give_event(static_cast<hipEvent_t>(r));
    }
    if (pl->dev_base) dev_pool().release(pl->dev_base, pl->dev_cap, pl->launched, static_cast<hipStream_t>(pl->last_stream));
    plan_pool().give(pl);
}

void bt_plan_pool_trim(void) { dev_pool().trim(); plan_pool().trim(); }

int bt_plan_get_info(const bt_plan *pl, bt_plan_info *info) {
    if (!pl || !info) return BT_EINVAL;
    *info = pl->info;
    return BT_OK;
}

size_t bt_plan_workspace_bytes(const bt_plan *pl) { return pl ? pl->ws.total : 0; }

// The tables bt_plan_array reads back from the plan's buffer: those the device wrote or amended (upload_plan), and every
// table of a shifted clone (clone_shifted: its host vectors are empty)
static bool device_written(const bt_plan *pl, int t) {
    if (!pl->dev_base) return false;
    if (pl->is_clone) return true;
    switch (t) {
    case tab::pm_edge: case tab::pm_rec: return pl->dev_pm != 0;
    case tab::slot_edge: case tab::slot_pair: case tab::slot_lab: case tab::slot_lp: case tab::tile_cut8: case tab::tile_cut16: return pl->dev_slots != 0;
    case tab::slot_code: case tab::tile_la: case tab::tile_rec: return pl->dev_slots && pl->dev_wpt;
    case tab::it_edge: case tab::tile_sinfo: return pl->dev_slots && pl->dev_wpt && pl->dev.em_ok;
    default: return false;
    }
}

int64_t bt_plan_array(const bt_plan *pl, const char *name, const void **data) {
    if (!pl || !name || !data) return -1;
    if (std::strcmp(name, "trk_loc") == 0) { *data = pl->trk_loc.data(); return (int64_t)pl->trk_loc.size(); }
    if (std::strcmp(name, "trk_of_patch") == 0) {            // kept for the window of patches only: expanded here (tests, tooling)
        pl->trk_of_patch.assign((size_t)pl->info.p_tot, -1);
        for (size_t i = 0; i < pl->trk_win.size(); ++i) pl->trk_of_patch[(size_t)pl->trk_win_lo + i] = pl->trk_win[i];
        *data = pl->trk_of_patch.data();
        return (int64_t)pl->trk_of_patch.size();
    }
    if (std::strcmp(name, "ws_layout") == 0) {                // byte offsets in the workspace: sys, zero_bytes, status, total (int64)
        const int64_t v[4] = {(int64_t)pl->ws.sys, (int64_t)pl->ws.zero_bytes, (int64_t)pl->ws.status, (int64_t)pl->ws.total};
        pl->dev_readback.assign(8, 0);
        std::memcpy(pl->dev_readback.data(), v, sizeof(v));
        *data = pl->dev_readback.data();
        return 4;
    }
    if (std::strcmp(name, "solver_mode") == 0) {              // 0 .. 3 (ba_plan.hpp: Route), -1 for a host-only plan
        pl->dev_readback.assign(1, pl->dev_base ? (int32_t)(pl->dev.route.solver >= Route::kSolveFused ? Route::kSolveLds : pl->dev.route.solver) : -1);
        *data = pl->dev_readback.data();
        return 1;
    }
    if (std::strcmp(name, "trk_off") == 0) {                  // sharded: distinct tracks in front of the rank's range (one element)
        pl->dev_readback.assign(1, (int32_t)pl->dev.trk_off);
        *data = pl->dev_readback.data();
        return 1;
    }
    // `count` elements of `esz` bytes at `off` of the plan's buffer, read back on request (tests, tooling).  A clone's copies
    // and shift kernels are queued on the plan stream, which is non-blocking: a hipMemcpy on the null stream is not ordered
    // behind it, so the stream is waited for (the plan's `ready` event is left alone: its hand-off is mark_launch's)
    const auto readback = [&](size_t off, size_t count, size_t esz) -> int64_t {
        const size_t bytes = count * esz;
        std::vector<int32_t> &r = pl->dev_readback;
        r.assign((bytes + 7) / 8 * 2, 0);
        if (pl->is_clone && hipStreamSynchronize(copy_stream()) != hipSuccess) return -1;
        if (bytes && hipMemcpy(r.data(), static_cast<const char *>(pl->dev_base) + off, bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        *data = r.data();
        return (int64_t)count;
    };
    if (std::strcmp(name, "edge_words") == 0)                 // the kept packed edge list (kk << 32 | ii << 16 | jj, uint64), empty where none is kept
        return readback(pl->pk_off, pl->dev_base && pl->pk_off ? (size_t)pl->dev.e_all : 0, sizeof(uint64_t));
    // an uploaded table: the host's vector, or — a table the device wrote, any table of a clone — the buffer's
    const auto table = [&](int t, const auto &v) -> int64_t {
        if (!device_written(pl, t)) { *data = v.data(); return (int64_t)v.size(); }
        return readback(pl->off[t], pl->len[t], sizeof(v[0]));
    };
#define BT_ARR(T, n, solver) if (std::strcmp(name, #n) == 0) return table(tab::n, pl->n);
    BT_PLAN_TABLES(BT_ARR)
#undef BT_ARR
    return -1;
}

int bt_ba_workspace_init(const bt_plan *pl, void *ws, void *stream) {
    if (!pl || !ws) return BT_EINVAL;
    char *w = static_cast<char *>(ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the accumulators, and the status block: kernels read its flags (the refinement's, the dense solver's) before they write them
    return hipMemsetAsync(w + pl->ws.sys, 0, pl->ws.zero_bytes, st) == hipSuccess && hipMemsetAsync(w + pl->ws.status, 0, kStatusBytes, st) == hipSuccess
               ? BT_OK : BT_EHIP;
}

int bt_ba_reduce(const bt_plan *pl, const bt_ba_args *a, void *ws, void *stream) {
    const int rc = check(pl, a, ws);
    if (rc != BT_OK) return rc;
    const StepArgs s = make_args(pl, a, ws);
    mark_launch(pl, stream);
    return launch_reduce(pl->dev, s, is_so(pl, a), static_cast<hipStream_t>(stream));
}

int bt_ba_solve_update(const bt_plan *pl, const bt_ba_args *a, void *ws, void *stream) {
    const StepMode m = step_mode(pl, a, ws);
    if (m.rc != BT_OK) return m.rc;
    const StepArgs s = make_args(pl, a, ws);
    mark_launch(pl, stream);
    return launch_solve_update(pl->dev, s, m.so, m.copy_poses, static_cast<hipStream_t>(stream));
}

int bt_ba_step(const bt_plan *pl, const bt_ba_args *a, void *ws, void *stream) {
    const StepMode m = step_mode(pl, a, ws);
    if (m.rc != BT_OK) return m.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    mark_launch(pl, stream);
    const StepArgs s = make_args(pl, a, ws);
    bool fused = false;              // (structure-only steps on the k_tile path are one launch)
    int r = launch_reduce(pl->dev, s, m.so, st, nullptr, nullptr, m.so ? (m.copy_poses ? 1 : 0) : -1, &fused);
    if (r == BT_OK && !fused) r = launch_solve_update(pl->dev, s, m.so, m.copy_poses, st, nullptr, nullptr, true);
    return r;
}

int bt_ba_step_timed(const bt_plan *pl, const bt_ba_args *a, void *ws, void *stream, float *ms) {
    const StepMode m = step_mode(pl, a, ws);
    if (m.rc != BT_OK || !ms) return m.rc != BT_OK ? m.rc : BT_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    mark_launch(pl, stream);
    hipEvent_t ev[12];
    for (auto &e : ev) if (hipEventCreate(&e) != hipSuccess) return BT_EHIP;
    const StepArgs s = make_args(pl, a, ws);
    unsigned ran = 0;
    int r = launch_reduce(pl->dev, s, m.so, st, ev, &ran);
    if (r == BT_OK) r = launch_solve_update(pl->dev, s, m.so, m.copy_poses, st, ev, &ran, true);
    if (r == BT_OK && hipStreamSynchronize(st) != hipSuccess) r = BT_EHIP;
    for (int k = 0; k < 6; ++k) {
        ms[k] = 0.0f;                                  // a kernel that was not launched (structure-only steps skip two) reads 0
        if (r == BT_OK && (ran >> k & 1u) && hipEventElapsedTime(&ms[k], ev[2 * k], ev[2 * k + 1]) != hipSuccess) ms[k] = -1.0f;
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    return r;
}

int bt_ba_pack(const bt_plan *pl, const bt_ba_args *a, void *ws, void *stream) {
    const int rc = check(pl, a, ws);
    if (rc != BT_OK) return rc;
    if (is_so(pl, a)) return BT_OK;
    mark_launch(pl, stream);
    return launch_pack(pl->dev, make_args(pl, a, ws), false, static_cast<hipStream_t>(stream));
}

int bt_ba_unpack(const bt_plan *pl, const bt_ba_args *a, void *ws, void *stream) {
    const int rc = check(pl, a, ws);
    if (rc != BT_OK) return rc;
    if (is_so(pl, a)) return BT_OK;
    mark_launch(pl, stream);
    return launch_pack(pl->dev, make_args(pl, a, ws), true, static_cast<hipStream_t>(stream));
}

int bt_ba_reduce_pack(const bt_plan *pl, const bt_ba_args *a, void *ws, void *stream) {
    const int rc = bt_ba_reduce(pl, a, ws, stream);
    return rc != BT_OK ? rc : bt_ba_pack(pl, a, ws, stream);
}

int bt_ba_unpack_solve_update(const bt_plan *pl, const bt_ba_args *a, void *ws, void *stream) {
    const int rc = bt_ba_unpack(pl, a, ws, stream);
    return rc != BT_OK ? rc : bt_ba_solve_update(pl, a, ws, stream);
}

size_t bt_xchg_bytes(const bt_plan *pl, int world) {
    return (pl && pl->dev_base && world > 0 && world <= kMaxRanks) ? xchg_bytes(pl->dev, world) : 0;
}

int bt_xchg_alloc(size_t bytes, void **buf, unsigned char handle[64]) {
    if (!buf || !handle || bytes == 0) return BT_EINVAL;
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
    void *d = nullptr;
    // uncached: the peers' stores and this rank's loads meet in memory, not in caches that are not coherent across dies / devices
    if (hipExtMallocWithFlags(&d, bytes, hipDeviceMallocUncached) != hipSuccess) return BT_ENOMEM;
    hipIpcMemHandle_t h;
    if (hipMemset(d, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipIpcGetMemHandle(&h, d) != hipSuccess) {
        (void)hipFree(d);
        return BT_EHIP;
    }
    std::memcpy(handle, &h, 64);
    *buf = d;
    return BT_OK;
}

int bt_config_wave_per_tile_kernels(int enable) { return bt::config_wave_per_tile_kernels(enable); }

int bt_xchg_open(const unsigned char handle[64], void **peer) {
    if (!handle || !peer) return BT_EINVAL;
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle, 64);
    return hipIpcOpenMemHandle(peer, h, hipIpcMemLazyEnablePeerAccess) == hipSuccess ? BT_OK : BT_EHIP;
}

int bt_xchg_close(void *peer) { return (!peer || hipIpcCloseMemHandle(peer) == hipSuccess) ? BT_OK : BT_EHIP; }
int bt_xchg_free(void *buf) { return (!buf || hipFree(buf) == hipSuccess) ? BT_OK : BT_EHIP; }

int bt_ba_reduce_push(const bt_plan *pl, const bt_ba_args *a, void *ws, void *const *bufs, int world, int rank, int64_t epoch, void *stream) {
    // (validated BEFORE anything is enqueued: an EINVAL must not leave half a step on the stream)
    if (!bufs || world < 1 || world > kMaxRanks || rank < 0 || rank >= world || epoch < 1) return BT_EINVAL;
    for (int q = 0; q < world; ++q) if (!bufs[q]) return BT_EINVAL;
    const int rc = bt_ba_reduce(pl, a, ws, stream);
    if (rc != BT_OK || is_so(pl, a)) return rc;
    return launch_xchg_push(pl->dev, make_args(pl, a, ws), bufs, world, rank, epoch, static_cast<hipStream_t>(stream));
}

int bt_ba_pull_solve_update(const bt_plan *pl, const bt_ba_args *a, void *ws, void *own, int world, int64_t epoch, void *stream) {
    const int rc = check(pl, a, ws);
    if (rc != BT_OK) return rc;
    if (!is_so(pl, a)) {
        if (!own || world < 1 || world > kMaxRanks || epoch < 1) return BT_EINVAL;
        mark_launch(pl, stream);
        const int r2 = launch_xchg_pull(pl->dev, make_args(pl, a, ws), own, world, epoch, static_cast<hipStream_t>(stream));
        if (r2 != BT_OK) return r2;
    }
    return bt_ba_solve_update(pl, a, ws, stream);
}

int bt_ba_xchg_status(const bt_plan *pl, void *ws, void *stream, int32_t *status) {
    if (!pl || !ws || !status) return BT_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemcpyAsync(status, static_cast<char *>(ws) + pl->ws.status + sizeof(int32_t), sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess)
        return BT_EHIP;
    return hipStreamSynchronize(st) == hipSuccess ? BT_OK : BT_EHIP;
}

double *bt_ba_packed(const bt_plan *pl, void *ws, int64_t *count) {
    if (!pl || !ws) return nullptr;
    if (count) *count = pl->info.nnz_blocks * 36 + 6 * pl->info.n;
    return reinterpret_cast<double *>(static_cast<char *>(ws) + pl->ws.packed);
}

double *bt_ba_system(const bt_plan *pl, void *ws, int64_t *count) {
    if (!pl || !ws) return nullptr;
    const int64_t D = 6 * pl->info.n;
    if (count) *count = D * D + D;
    return reinterpret_cast<double *>(static_cast<char *>(ws) + pl->ws.sys);
}

float *bt_ba_dx(const bt_plan *pl, void *ws) {
    return (pl && ws) ? reinterpret_cast<float *>(static_cast<char *>(ws) + pl->ws.dx) : nullptr;
}

int bt_ba_status(const bt_plan *pl, void *ws, void *stream, int32_t *status) {
    if (!pl || !ws || !status) return BT_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t w[3] = {0, 0, 0};             // (the solver's word, the exchange's, the fused update's hand-off time-out)
    if (hipMemcpyAsync(w, static_cast<char *>(ws) + pl->ws.status, sizeof(w), hipMemcpyDeviceToHost, st) != hipSuccess)
        return BT_EHIP;
    if (hipStreamSynchronize(st) != hipSuccess) return BT_EHIP;
    *status = w[kStatusHandoff] != 0 ? w[kStatusHandoff] : w[0];
    return BT_OK;
}

}  // extern "C"
