// plan_shift.cpp — the shifted clones of the C ABI (include/batrack_ba.h): the plan of an edge list that is an earlier plan's with
// every frame number moved by one constant and every patch number by another, made from that plan's tables on the device.
// Who may be a source, which shifts fit, the delta word and the speculation states are each stated once, below.
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>

#include "plan_host.hpp"

namespace bt {

// May `src` be the source of a clone for a list of E edges in buffers of n_buf frames / p_tot patches: uploaded, its packed list
// kept and the whole of it (e_all == info.E: not a rank's share), the same buffers, and no speculation that is still unsettled
static bool shift_source(const bt_plan *src, int64_t E, int64_t n_buf, int64_t p_tot) {
    return src->dev_base && src->pk_off && src->dev.e_all == E && src->info.E == E && src->info.n_buf == n_buf &&
           src->info.p_tot == p_tot && !src->spec.unsettled();
}

// Does a shift of `src` by df frames fit its buffers BEFORE the new list is known: every number the clone's tables will hold
// stays inside them, whatever that list turns out to be.  Returns dk, the patches the shift moves by (> 0), or -1.
static int64_t shift_fits(const bt_plan *src, int64_t df) {
    const int64_t n_buf = src->info.n_buf, p_tot = src->info.p_tot;
    if (n_buf <= 0 || p_tot % n_buf != 0) return -1;           // (dk is derived: a frame must own a whole number of patches)
    const int64_t dk = df * (p_tot / n_buf);
    return df > 0 && df < 32768 && src->info.n_all + df <= n_buf && src->k_hi >= 0 && src->k_hi + dk < p_tot ? dk : -1;
}

// The delta word: what every packed edge word (kk << 32 | ii << 16 | jj) grows by under a shift of di frames / dk patches
struct Shift { int64_t di, dj, dk; };                          // (dj: the target frames' shift — a shifted copy has dj == di)
static uint64_t delta_word(int64_t di, int64_t dk) { return ((uint64_t)dk << 32) | ((uint64_t)di << 16) | (uint64_t)di; }
static Shift delta_parts(uint64_t d) { return {(int64_t)((d >> 16) & 0xffff), (int64_t)(d & 0xffff), (int64_t)(d >> 32)}; }

// the packed edge list a shift source keeps behind its tables
static const uint64_t *kept_words(const bt_plan *pl) { return reinterpret_cast<const uint64_t *>(static_cast<const char *>(pl->dev_base) + pl->pk_off); }

// The clone of `src` for a list shifted by di frames / dk patches: tables copied and shifted on the plan stream `cs` (the new list's
// packed words, d_words, behind them), no host wait — the plan carries the event its first launches are ordered behind.
static int clone_shifted(const bt_plan *src, const uint64_t *d_words, int64_t E, int64_t fixedp, int64_t di, int64_t dk, hipStream_t cs, bt_plan **out) {
    PhaseTimer tick{"plan api"};
    bt_plan *pl = plan_pool().take();
    if (!pl) return BT_ENOMEM;
    // (its dev_pm / dev_slots / dev_wpt stay 0: every table of the clone is in its buffer, none is written there by a planner pass)
    pl->info = src->info; pl->info.fixedp = fixedp; pl->info.n_all = src->info.n_all + di;
    pl->ws = src->ws; pl->off = src->off; pl->len = src->len; pl->dev_bytes = src->dev_bytes; pl->pk_off = src->pk_off; pl->pm_rounds = src->pm_rounds;
    pl->dev = src->dev;
    pl->is_clone = 1;
    pl->k_hi = src->k_hi >= 0 ? src->k_hi + dk : -1;
    size_t cap = 0;
    void *d = dev_pool().acquire(pl->dev_bytes + 256, cs, &cap);
    if (!d) { plan_pool().give(pl); return BT_ENOMEM; }
    char *nb = static_cast<char *>(d);
    const char *ob = static_cast<const char *>(src->dev_base);
    auto I32 = [&](int t) { return reinterpret_cast<int32_t *>(nb + pl->off[t]); };
    int rc = BT_OK;
    // the tables as they are, the new packed edge list behind them, then the ones that hold absolute frame / patch numbers
    // (d_words null — a clone made ahead of its list, bt_plan_preshift: the list it expects, the source's words moved by the shift)
    if (hipMemcpyAsync(nb, ob, src->pk_off, hipMemcpyDeviceToDevice, cs) != hipSuccess) rc = BT_EHIP;
    else if (d_words) { if (hipMemcpyAsync(nb + pl->pk_off, d_words, (size_t)E * sizeof(uint64_t), hipMemcpyDeviceToDevice, cs) != hipSuccess) rc = BT_EHIP; }
    else rc = launch_words_add(kept_words(src), delta_word(di, dk), reinterpret_cast<uint64_t *>(nb + pl->pk_off), E, cs);
    if (rc == BT_OK)
        rc = launch_plan_shift(I32(tab::kx), (int)pl->info.m, I32(tab::tile_kx), (int)pl->info.tiles * kLanes, I32(tab::tile_ij), (int)pl->len[tab::tile_ij],
                               I32(tab::pair_i), I32(tab::pair_j), (int)pl->info.pairs, reinterpret_cast<const uint32_t *>(ob + pl->off[tab::act_bits]),
                               reinterpret_cast<uint32_t *>(nb + pl->off[tab::act_bits]), I32(tab::act_rank), (int)pl->len[tab::act_bits], (int)di, (int)dk, cs);
    // no host wait for the copies: the plan's first launches are ordered behind this event on whatever stream they use
    hipEvent_t ready = rc == BT_OK ? dev_pool().take_event() : nullptr;
    if (rc == BT_OK && (!ready || hipEventRecord(ready, cs) != hipSuccess)) {
        dev_pool().give_event(ready); ready = nullptr;
        if (hipStreamSynchronize(cs) != hipSuccess) rc = BT_EHIP;
    }
    tick("shifted: copies enqueued");
    if (rc != BT_OK) { (void)hipStreamSynchronize(cs); dev_pool().release(d, cap, false, nullptr); plan_pool().give(pl); return rc; }
    pl->ready = ready;
    pl->dev_base = d;
    pl->dev_cap = cap;
    bind_pointers(pl, d);
    rc = configure_kernels(pl->dev);
    tick("shifted: configure kernels");
    if (rc != BT_OK) { bt_plan_destroy(pl); return rc; }
    *out = pl;
    return BT_OK;
}

// Verdicts of speculative clones: pinned / device int pairs handed out round robin (a plan's verdict is read by
// bt_plan_spec_confirm right after its first step; sixteen unconfirmed speculative plans at a time are sixteen more than the
// caller has)
struct SpecSlots {
    static constexpr unsigned kSlots = 16;
    static constexpr int kFlagInts = 4;                                      // ints a slot (SpecState::flag: three used)
    int *h = nullptr;                                                        // pinned, mapped: the comparison kernel writes its verdict there
    unsigned *tickets[kMaxDevices] = {};                                     // device memory, per device: one counter a slot (k_match_done's last-workgroup ticket)
    hipEvent_t ev_in = nullptr;                                              // orders the plan stream behind the caller's stream
    unsigned next = 0;                                                       // slot = next++ % kSlots, its flags at h + kFlagInts * slot
    bool ensure() {
        if (h && ev_in) return true;
        constexpr size_t bytes = kSlots * kFlagInts * sizeof(int);
        if (!h) { if (hipHostMalloc(reinterpret_cast<void **>(&h), bytes, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent) != hipSuccess) return false; std::memset(h, 0, bytes); }
        return ev_in || hipEventCreateWithFlags(&ev_in, hipEventDisableTiming) == hipSuccess;
    }
    // the tickets of the device a plan lives on (allocated on first use, with that device current — as it is for every launch of the plan)
    unsigned *tickets_of(int dev) {
        if (dev < 0 || dev >= kMaxDevices) return nullptr;
        if (!tickets[dev] && (hipMalloc(reinterpret_cast<void **>(&tickets[dev]), kSlots * sizeof(unsigned)) != hipSuccess ||
                              hipMemset(tickets[dev], 0, kSlots * sizeof(unsigned)) != hipSuccess)) { tickets[dev] = nullptr; return nullptr; }
        return tickets[dev];
    }
};
static SpecSlots &spec_slots() { static SpecSlots s; return s; }
static std::mutex &spec_mutex() { static std::mutex m; return m; }

}  // namespace bt

using namespace bt;

extern "C" {

int bt_plan_create_shifted_spec(const bt_plan *src, const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E,
                                int64_t n_buf, int64_t p_tot, int64_t fixedp, void *in_stream, bt_plan **out) {
    if (!out) return BT_EINVAL;
    *out = nullptr;
    if (!src || !ii || !jj || !kk || E <= 0) return BT_EINVAL;
    // (one source, named by the caller: one that is not eligible is an answer — bt_plan_create_shifted_any skips it and looks on)
    if (!buffers_packable(n_buf, p_tot) || !shift_source(src, E, n_buf, p_tot)) return BT_NO_MATCH;
    const int64_t di = fixedp - src->info.fixedp, dk = shift_fits(src, di);
    if (dk < 0) return BT_NO_MATCH;
    PhaseTimer tick{"plan api"};
    PackBuffers &pb = pack_buffers();
    if (!pb.ensure((size_t)E)) return BT_ENOMEM;
    int *h_flag;
    hipStream_t cs = copy_stream();
    {
        std::lock_guard<std::mutex> g(spec_mutex());
        SpecSlots &ss = spec_slots();
        if (!ss.ensure()) return BT_ENOMEM;
        h_flag = ss.h + SpecSlots::kFlagInts * (ss.next++ % SpecSlots::kSlots);
        // the index tensors are complete when `in_stream` gets here: the plan stream waits for that, the host does not
        if (hipEventRecord(ss.ev_in, static_cast<hipStream_t>(in_stream)) != hipSuccess || hipStreamWaitEvent(cs, ss.ev_in, 0) != hipSuccess) {
            if (hipStreamSynchronize(static_cast<hipStream_t>(in_stream)) != hipSuccess) return BT_EHIP;
        }
    }
    h_flag[0] = 0; h_flag[1] = 0;
    hipEvent_t spec_ev = dev_pool().take_event();
    if (!spec_ev) return BT_ENOMEM;
    const bool ok = launch_pack_match_expect(ii, jj, kk, E, n_buf, p_tot, kept_words(src), delta_word(di, dk), pb.d_words, h_flag, cs) == BT_OK &&
                    hipEventRecord(spec_ev, cs) == hipSuccess;
    if (!ok) { (void)hipStreamSynchronize(cs); dev_pool().give_event(spec_ev); return BT_EHIP; }
    tick("speculative shift: pack + match enqueued");
    bt_plan *pl = nullptr;
    const int rc = clone_shifted(src, pb.d_words, E, fixedp, di, dk, cs, &pl);
    if (rc != BT_OK) { (void)hipEventSynchronize(spec_ev); dev_pool().give_event(spec_ev); return rc; }
    pl->spec.state = SpecState::kEvent; pl->spec.event = spec_ev; pl->spec.flag = h_flag;
    *out = pl;
    return BT_OK;
}

// The two halves of bt_plan_create_shifted_spec apart.  The caller's window moves by the same number of frames update() after
// update(): the clone for the NEXT list can be made while the steps of the current one run (its tables depend on the source and
// the shift only), and what is left for the call that brings the list — the first of an update(), with the GPU idle behind it — is
// the comparison kernel.
int bt_plan_preshift(const bt_plan *src, int64_t df, bt_plan **out) {
    if (!out) return BT_EINVAL;
    *out = nullptr;
    if (!src) return BT_EINVAL;
    // (the list does not exist yet: the clone is for the source's own size and buffers)
    const int64_t n_buf = src->info.n_buf, p_tot = src->info.p_tot, E = src->dev.e_all;
    if (E <= 0 || !buffers_packable(n_buf, p_tot) || !shift_source(src, E, n_buf, p_tot)) return BT_NO_MATCH;
    const int64_t dk = shift_fits(src, df);
    if (dk < 0) return BT_NO_MATCH;
    bt_plan *pl = nullptr;
    const int rc = clone_shifted(src, nullptr, E, src->info.fixedp + df, df, dk, copy_stream(), &pl);
    if (rc != BT_OK) return rc;
    pl->spec.state = SpecState::kUnbound;
    *out = pl;
    return BT_OK;
}

int bt_plan_spec_bind(bt_plan *pl, const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E, int64_t n_buf, int64_t p_tot,
                      int64_t fixedp, void *in_stream) {
    if (!pl || !ii || !jj || !kk) return BT_EINVAL;
    if (pl->spec.state != SpecState::kUnbound || !pl->dev_base) return BT_EINVAL;
    if (pl->dev.e_all != E || pl->info.n_buf != n_buf || pl->info.p_tot != p_tot || pl->info.fixedp != fixedp) return BT_NO_MATCH;
    PhaseTimer tick{"plan api"};
    int *h_flag;
    unsigned *ticket;
    int epoch;
    {
        std::lock_guard<std::mutex> g(spec_mutex());
        SpecSlots &ss = spec_slots();
        if (!ss.ensure()) return BT_ENOMEM;
        unsigned *tk = ss.tickets_of(pl->dev.dev_id);
        if (!tk) return BT_ENOMEM;
        const unsigned slot = ss.next++ % SpecSlots::kSlots;
        h_flag = ss.h + SpecSlots::kFlagInts * slot; ticket = tk + slot;
        epoch = (int)((ss.next & 0x3fffffffu) | 0x40000000u);          // (never 0, never the slot's previous one)
    }
    h_flag[0] = 0; h_flag[1] = 0; h_flag[2] = 0;
    // the list against the one the clone was made for (its own packed words): ONE launch, on the stream that made the index tensors
    // and will run the step — no cross-stream order to set up, no event to record (the verdict is polled: bt_plan_spec_confirm)
    if (launch_match_done(ii, jj, kk, E, n_buf, p_tot, kept_words(pl), h_flag, ticket, epoch, in_stream) != BT_OK) return BT_EHIP;
    tick("bind: comparison launched");
    pl->spec.state = SpecState::kPolled; pl->spec.flag = h_flag; pl->spec.epoch = epoch; pl->spec.stream = in_stream;
    return BT_OK;
}

int bt_plan_spec_confirm(bt_plan *pl) {
    if (!pl) return BT_EINVAL;
    SpecState &sp = pl->spec;
    volatile int *f = sp.flag;
    bool done = false;
    switch (sp.state) {
    case SpecState::kNone: return BT_OK;
    case SpecState::kUnbound: return BT_NO_MATCH;                // (never given its list)
    case SpecState::kPolled: {
        // (bt_plan_spec_bind: the comparison ran in front of the step that was just enqueued; its last workgroup wrote the epoch)
        const int want = sp.epoch;
        for (int spins = 0; spins < (1 << 17) && !done; ++spins) done = f[2] == want;      // (~ 2 ms)
        if (!done) {
            // a GPU far behind — the caller's earlier work sits in front of the comparison: keep looking, but let the core go in
            // between (returning when the VERDICT is there, not when the step behind it is done, keeps the next call's launches
            // under that step); after seconds of that, the stream itself
            const auto t0 = std::chrono::steady_clock::now();
            while (!(done = f[2] == want) && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(5)) std::this_thread::yield();
            if (!done) {
                if (hipStreamSynchronize(static_cast<hipStream_t>(sp.stream)) != hipSuccess) return BT_EHIP;
                done = f[2] == want;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        break;
    }
    case SpecState::kEvent: {
        hipEvent_t ev = static_cast<hipEvent_t>(sp.event);
        done = hipEventSynchronize(ev) == hipSuccess;
        dev_pool().give_event(ev);
        break;
    }
    }
    // the verdict, for either way of waiting: settled whatever it says
    const int differs = f[0], bad = f[1];
    sp = SpecState{};
    if (!done) return BT_EHIP;
    if (bad) return BT_EINVAL;
    return differs ? BT_NO_MATCH : BT_OK;
}

// The plan of a list that is a shifted copy of ONE of up to four earlier plans' lists (the caller's cache, most likely first):
// packed once, compared with every candidate in the same queue, one synchronisation for all of them (a candidate that does not
// match used to cost a round trip of its own: with a keyframe stride of 2 every other update of the replay paid one).  The clone's
// tables are copied and shifted on the plan stream WITHOUT a host wait: the plan carries an event (`ready`) that its first
// launches are ordered behind (mark_launch).
int bt_plan_create_shifted_any(const bt_plan *const *srcs, int nsrc, const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E,
                               int64_t n_buf, int64_t p_tot, int64_t fixedp, int *which, bt_plan **out) {
    if (!out) return BT_EINVAL;
    *out = nullptr;
    if (which) *which = -1;
    if (!srcs || nsrc <= 0 || !ii || !jj || !kk || E <= 0) return BT_EINVAL;
    if (!buffers_packable(n_buf, p_tot)) return BT_NO_MATCH;
    const bt_plan *cand[kMaxShiftSources];
    int idx[kMaxShiftSources], nc = 0;
    for (int q = 0; q < nsrc && nc < kMaxShiftSources; ++q) {
        const bt_plan *src = srcs[q];
        if (!src) return BT_EINVAL;
        // (several candidates: one that is not eligible is skipped, where bt_plan_create_shifted_spec answers BT_NO_MATCH for its one)
        if (!shift_source(src, E, n_buf, p_tot)) continue;
        cand[nc] = src; idx[nc++] = q;
    }
    if (nc == 0) return BT_NO_MATCH;
    PhaseTimer tick{"plan api"};
    PackBuffers &pb = pack_buffers();
    if (!pb.ensure((size_t)E, /*cmp=*/true)) return BT_ENOMEM;
    constexpr int kCmpInts = PackBuffers::kCmpInts;
    hipStream_t cs = copy_stream();
    int *d_bad = pb.d_cmp + 4 * kMaxShiftSources;
    bool ok = hipMemsetAsync(pb.d_cmp, 0, kCmpInts * sizeof(int), cs) == hipSuccess &&
              launch_pack_edges(ii, jj, kk, E, n_buf, p_tot, pb.d_words, d_bad, cs) == BT_OK;
    for (int q = 0; ok && q < nc; ++q) {
        ok = launch_shift_match(pb.d_words, kept_words(cand[q]), E, pb.d_cmp + 4 * q, cs) == BT_OK;
    }
    if (!ok || hipMemcpyAsync(pb.h_cmp, pb.d_cmp, kCmpInts * sizeof(int), hipMemcpyDeviceToHost, cs) != hipSuccess ||
        hipStreamSynchronize(cs) != hipSuccess)
        return BT_EHIP;
    tick("shifted: pack + match (synchronised)");
    if (pb.h_cmp[4 * kMaxShiftSources]) return BT_EINVAL;
    const bt_plan *src = nullptr;
    Shift s{0, 0, 0};
    for (int q = 0; q < nc && !src; ++q) {
        const int *c = pb.h_cmp + 4 * q;
        if (c[0]) continue;
        s = delta_parts((uint64_t)(uint32_t)c[2] | ((uint64_t)(uint32_t)c[3] << 32));
        // (shifts forward in time only; both frame fields by the same amount; the fixed prefix moves along)
        // (not shift_fits: di and dk are MEASURED on a list that was range-checked above, so the patches need no k_hi test and
        //  n_buf no divisibility; what the list does not show is that the window's frames stay inside n_buf)
        if (s.di != s.dj || s.dk >= ((int64_t)1 << 31) || fixedp != cand[q]->info.fixedp + s.di || cand[q]->info.n_all + s.di > n_buf) continue;
        if (s.di == 0 && s.dk == 0) continue;                       // the same list: the caller's cache has that plan already
        src = cand[q];
        if (which) *which = idx[q];
    }
    if (!src) return BT_NO_MATCH;
    return clone_shifted(src, pb.d_words, E, fixedp, s.di, s.dk, cs, out);
}

int bt_plan_create_shifted(const bt_plan *src, const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E,
                           int64_t n_buf, int64_t p_tot, int64_t fixedp, bt_plan **out) {
    if (!out) return BT_EINVAL;
    *out = nullptr;
    if (!src) return BT_EINVAL;
    return bt_plan_create_shifted_any(&src, 1, ii, jj, kk, E, n_buf, p_tot, fixedp, nullptr, out);
}

}  // extern "C"
