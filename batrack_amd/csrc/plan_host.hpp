// plan_host.hpp — what the two host units behind the plan entry points of the C ABI share: ba_api.cpp (the pools' instances,
// upload_plan, create / destroy, the step entry points) and plan_shift.cpp (the shifted clones).  No kernel includes this.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "ba_kernels.hpp"

namespace bt {

// Device buffers of destroyed plans are kept for the next plan: the caller replaces its edge list every frame
// (batrack.py:189-212), so a plan lives for 2*ITER steps, and hipMalloc / hipFree per frame is what a frame
// would otherwise wait for (hipFree synchronises the device and unmaps).  Sizes are rounded up so that the
// slowly varying edge count of a sliding window maps onto the same bucket.
struct DevPool {
    struct Entry { void *p; size_t cap; hipEvent_t ev; bool pending; };   // ev: recorded behind the last kernels that read the buffer
    std::mutex mu;
    std::vector<Entry> free_list;
    static size_t bucket(size_t bytes) {           // 12.5 % head room, whole MiB, at least 2 MiB
        const size_t g = (size_t)1 << 20;
        return std::max<size_t>(2 * g, (bytes + bytes / 8 + g - 1) / g * g);
    }
    // A buffer of at least `bytes` (*cap: what it holds) that stream `cs` may write.  nullptr: out of memory.
    void *acquire(size_t bytes, hipStream_t cs, size_t *cap) {
        const size_t want = bucket(bytes);
        Entry e{nullptr, want, nullptr, false};
        {
            std::lock_guard<std::mutex> lk(mu);
            size_t best = free_list.size();
            for (size_t i = 0; i < free_list.size(); ++i)
                if (free_list[i].cap >= bytes && free_list[i].cap <= 2 * want &&
                    (best == free_list.size() || free_list[i].cap < free_list[best].cap)) best = i;
            if (best != free_list.size()) { e = free_list[best]; free_list.erase(free_list.begin() + (long)best); }
        }
        // a recycled buffer may still be read by kernels of the destroyed plan queued on the caller's stream: the writes of `cs`
        // are ordered behind them on the device (no host wait, unless that cannot be enqueued)
        if (e.pending && hipStreamWaitEvent(cs, e.ev, 0) != hipSuccess) (void)hipEventSynchronize(e.ev);
        give_event(e.ev);
        if (!e.p && hipMalloc(&e.p, want) != hipSuccess) return nullptr;
        *cap = e.cap;
        return e.p;
    }
    std::vector<hipEvent_t> spare;                 // events not attached to a buffer (guarded by mu)
    void give_event(hipEvent_t ev) { if (ev) { std::lock_guard<std::mutex> lk(mu); spare.push_back(ev); } }
    hipEvent_t take_event() {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!spare.empty()) { hipEvent_t ev = spare.back(); spare.pop_back(); return ev; }
        }
        hipEvent_t ev = nullptr;
        return hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess ? ev : nullptr;
    }
    // last_stream != nullptr / launched: kernels reading the buffer may still be queued there
    void release(void *p, size_t cap, bool launched, hipStream_t last_stream) {
        Entry e{p, cap, nullptr, false};
        if (launched) {
            e.ev = take_event();
            if (e.ev && hipEventRecord(e.ev, last_stream) == hipSuccess) e.pending = true;
            else (void)hipStreamSynchronize(last_stream);            // no event: the plain hipFree this pool replaces synchronised too
        }
        void *drop = nullptr;
        hipEvent_t drop_ev = nullptr;
        {
            std::lock_guard<std::mutex> lk(mu);
            free_list.push_back(e);
            if (free_list.size() > 8) {            // keep the eight largest
                size_t sm = 0;
                for (size_t i = 1; i < free_list.size(); ++i) if (free_list[i].cap < free_list[sm].cap) sm = i;
                drop = free_list[sm].p; drop_ev = free_list[sm].ev;
                free_list.erase(free_list.begin() + (long)sm);
            }
        }
        if (drop) (void)hipFree(drop);             // (hipFree waits for the device: nothing can still read the buffer)
        if (drop_ev) (void)hipEventDestroy(drop_ev);
    }
    void trim() {
        std::vector<Entry> all;
        std::vector<hipEvent_t> evs;
        { std::lock_guard<std::mutex> lk(mu); all.swap(free_list); evs.swap(spare); }
        for (auto &e : all) { (void)hipFree(e.p); if (e.ev) (void)hipEventDestroy(e.ev); }
        for (auto ev : evs) (void)hipEventDestroy(ev);
    }
};
DevPool &dev_pool();

// Destroyed plan objects, vectors emptied but not released (bt_plan::recycle).
struct PlanPool {
    std::mutex mu;
    std::vector<bt_plan *> idle;
    bt_plan *take() {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!idle.empty()) { bt_plan *p = idle.back(); idle.pop_back(); return p; }
        }
        return new (std::nothrow) bt_plan();
    }
    void give(bt_plan *p) {
        p->recycle();
        {
            std::lock_guard<std::mutex> lk(mu);
            if (idle.size() < 8) { idle.push_back(p); return; }
        }
        delete p;
    }
    void trim() {
        std::vector<bt_plan *> all;
        { std::lock_guard<std::mutex> lk(mu); all.swap(idle); }
        for (bt_plan *p : all) delete p;
    }
};
PlanPool &plan_pool();

// The stream of the plan transfers (index download, table upload, a clone's copies), one per device, non-blocking
hipStream_t copy_stream();

// tile_ij packs two frame numbers into a signed 32-bit word, the packed edge list a patch number into 32 bits: buffers
// beyond these have no packed list on the device, so neither a plan built from one there nor a shifted clone
inline bool buffers_packable(int64_t n_buf, int64_t p_tot) { return n_buf <= 32768 && p_tot <= (int64_t)0x7fffffff; }

// the candidates one call of bt_plan_create_shifted_any compares the new list with
constexpr int kMaxShiftSources = 4;

// Per host thread: device words + flag and their pinned host mirror for the packed edge list (grown, never shrunk)
struct PackBuffers {
    static constexpr int kCmpInts = 4 * kMaxShiftSources + 4;     // per candidate: mismatch, -, shift lo, shift hi; then the range check's verdict
    uint64_t *d_words = nullptr, *h_words = nullptr;
    int *d_bad = nullptr, *h_bad = nullptr;
    int *d_cmp = nullptr, *h_cmp = nullptr;                  // result of the shift comparison (bt_plan_create_shifted_any), kCmpInts each
    size_t cap = 0;
    // room for n words; `cmp`: and d_cmp / h_cmp (made on first use)
    bool ensure(size_t n, bool cmp = false) {
        if (cmp && !d_cmp && hipMalloc(reinterpret_cast<void **>(&d_cmp), kCmpInts * sizeof(int)) != hipSuccess) return false;
        if (cmp && !h_cmp && hipHostMalloc(reinterpret_cast<void **>(&h_cmp), kCmpInts * sizeof(int), hipHostMallocDefault) != hipSuccess) return false;
        if (n <= cap && d_words) return true;
        if (d_words) { (void)hipFree(d_words); (void)hipHostFree(h_words); d_words = nullptr; h_words = nullptr; cap = 0; }
        const size_t want = n + n / 4 + 4096;
        if (hipMalloc(reinterpret_cast<void **>(&d_words), want * sizeof(uint64_t)) != hipSuccess) return false;
        if (hipHostMalloc(reinterpret_cast<void **>(&h_words), want * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) return false;
        if (!d_bad && hipMalloc(reinterpret_cast<void **>(&d_bad), sizeof(int)) != hipSuccess) return false;
        if (!h_bad && hipHostMalloc(reinterpret_cast<void **>(&h_bad), sizeof(int), hipHostMallocDefault) != hipSuccess) return false;
        cap = want;
        return true;
    }
};
PackBuffers &pack_buffers();

// PlanDev's figures of the plan info and its table pointers, for tables that sit at `d` as pl->off places them (upload_plan,
// clone_shifted); its other scalars are the planner's and upload_plan's
void bind_pointers(bt_plan *pl, const void *d);

}  // namespace bt
