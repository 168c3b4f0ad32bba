// plan_dump.cpp — the host planner's whole output as text, for comparing two trees bit by bit (no HIP, no GPU).
//
//   g++ -std=c++17 -O2 tools/plan_dump.cpp batrack_amd/csrc/ba_plan*.cpp -o plan_dump
//   python tools/plan_corpus.py corpus.bin && ./plan_dump corpus.bin > new.txt        (BT_FORCE as wanted: parsed once per process)
//   ./plan_dump corpus.bin --time 9                                                   (median ms per build, modes 1 and 3)
//
// It uses only what ba_plan.hpp declares, so the same source builds against a worktree of another commit.  Sanitizers: add
// -fsanitize=address,undefined -g to the line above and run it the same way.
//
// corpus.bin: cases one after the other, each int64 E, n_buf, p_tot, fixedp, n_all_min, own_lo, own_hi, then ii[E], jj[E], kk[E]
// (int64).  Per case build_plan_host runs in three modes — 1: edges, the uploaded plan; 2: edges, keep_slots (Plan(upload=False));
// 3: a DevPlanStats filled here from the same edges as plan_device.hip fills it (PatchStat / RepStat as ba_plan.hpp defines them,
// rep_known = 1), which reaches the planner's dstats branches — and, for a case with an own range, 4: mode 3 with the table
// sliced to the range and the coupling pattern of the whole list.  Per call: the return code and, where it is BT_OK, every
// scalar the planner sets and length + FNV-1a hash of every table.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../batrack_amd/csrc/ba_plan.hpp"

using namespace bt;

struct Case { int64_t E, n_buf, p_tot, fixedp, n_all_min, own_lo, own_hi; std::vector<int64_t> ii, jj, kk; };

static bool read_case(FILE *f, Case &c) {
    int64_t h[7];
    if (std::fread(h, sizeof(int64_t), 7, f) != 7) return false;
    c.E = h[0]; c.n_buf = h[1]; c.p_tot = h[2]; c.fixedp = h[3]; c.n_all_min = h[4]; c.own_lo = h[5]; c.own_hi = h[6];
    for (auto *v : {&c.ii, &c.jj, &c.kk}) {
        v->resize((size_t)c.E);
        if (c.E && std::fread(v->data(), sizeof(int64_t), (size_t)c.E, f) != (size_t)c.E) return false;
    }
    return true;
}

// the device's per-track table from the host's edges; ok = false where plan_device_stats answers BT_NEED_EDGES itself
struct Stats {
    std::vector<PatchStat> tab; std::vector<RepStat> rtab; std::vector<uint32_t> pattern;
    DevPlanStats st{}; bool ok = true;
};
static void fill_stats(const Case &c, bool sliced, Stats &s) {
    s = Stats{};
    if (c.E <= 0) return;                                 // (an empty table: the planner itself answers BT_NEED_EDGES)
    int64_t kmin = c.p_tot, kmax = -1, n_all = 0, f_lo = c.n_buf; int any_self = 0;
    for (int64_t e = 0; e < c.E; ++e) {
        if (c.ii[e] < 0 || c.jj[e] < 0 || c.ii[e] >= c.n_buf || c.jj[e] >= c.n_buf || c.kk[e] < 0 || c.kk[e] >= c.p_tot) { s.ok = false; return; }
        kmin = std::min(kmin, c.kk[e]); kmax = std::max(kmax, c.kk[e]);
        n_all = std::max(n_all, std::max(c.ii[e], c.jj[e]) + 1); f_lo = std::min(f_lo, std::min(c.ii[e], c.jj[e]));
        any_self |= c.ii[e] == c.jj[e];
    }
    std::vector<PatchStat> full((size_t)(kmax - kmin + 1), PatchStat{0, -1, 0x7fffffff, 0, 0ull, 0ull});
    std::vector<RepStat> rep(full.size(), RepStat{0ull, 0ull});
    bool any_rep = false;
    for (int64_t e = 0; e < c.E; ++e) {
        PatchStat &t = full[(size_t)(c.kk[e] - kmin)];
        ++t.cnt; t.src = std::max(t.src, (int32_t)c.ii[e]); t.src_min = std::min(t.src_min, (int32_t)c.ii[e]);
    }
    for (int64_t e = 0; e < c.E; ++e) {
        PatchStat &t = full[(size_t)(c.kk[e] - kmin)];
        RepStat &r = rep[(size_t)(c.kk[e] - kmin)];
        if (t.src != t.src_min) { s.ok = false; return; }                      // two source frames for a track
        const int64_t bit = c.jj[e] - ((int64_t)t.src - 64);
        if (bit < 0 || bit >= 128) { s.ok = false; return; }                    // a target outside the mask
        unsigned long long &mw = bit < 64 ? t.mask : t.mask2, &rw = bit < 64 ? r.rmask : r.rmask2;
        if (mw & (1ull << (bit & 63))) { rw |= 1ull << (bit & 63); any_rep = true; }
        mw |= 1ull << (bit & 63);
    }
    DevPlanStats &st = s.st;
    st.kmin = kmin; st.kmax = kmax; st.n_all = n_all; st.f_lo = f_lo; st.any_self = any_self; st.rep_known = 1;
    int64_t lo = kmin, hi = kmax + 1;
    if (sliced) {
        lo = std::min(std::max(c.own_lo, kmin), kmax + 1); hi = std::max(lo, std::min(c.own_hi, kmax + 1));
        st.sliced = 1;
        for (int64_t k = kmin; k < lo; ++k) if (full[(size_t)(k - kmin)].cnt > 0) { ++st.trk_before; st.edges_before += full[(size_t)(k - kmin)].cnt; }
        const int64_t n = std::max<int64_t>(std::max(n_all, c.n_all_min) - c.fixedp, 0);
        if (n > 0 && n <= kMaxFree) {
            const int words = (int)((n + 31) / 32);
            s.pattern.assign((size_t)n * words, 0u);
            std::vector<int64_t> cs;
            for (const PatchStat &t : full) {
                if (t.cnt <= 0) continue;
                cs.clear();
                if (t.src >= c.fixedp) cs.push_back(t.src - c.fixedp);
                for (int b = 0; b < 128; ++b)
                    if (((b < 64 ? t.mask : t.mask2) >> (b & 63)) & 1ull) { const int64_t fr = (int64_t)t.src - 64 + b - c.fixedp; if (fr >= 0) cs.push_back(fr); }
                for (int64_t u : cs) for (int64_t v : cs) if (u >= v) s.pattern[(size_t)u * words + (size_t)(v >> 5)] |= 1u << (v & 31);
            }
            st.pattern = s.pattern.data(); st.pattern_words = words;
        }
    }
    s.tab.assign(full.begin() + (lo - kmin), full.begin() + (hi - kmin));
    s.rtab.assign(rep.begin() + (lo - kmin), rep.begin() + (hi - kmin));
    st.tab = s.tab.data(); st.tab_lo = lo; st.tab_n = hi - lo; st.rtab = any_rep ? s.rtab.data() : nullptr;
}

template <class T> static void dump_vec(const char *name, const std::vector<T> &v) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) { h ^= p[i]; h *= 1099511628211ull; }
    std::printf(" %s=%zu:%016llx", name, v.size(), (unsigned long long)h);
}

static void dump_plan(const bt_plan &pl) {
    const bt_plan_info &I = pl.info;
    std::printf("  info E=%lld n_buf=%lld p_tot=%lld fixedp=%lld n_all=%lld n=%lld m=%lld pairs=%lld tiles=%lld slots=%lld erows=%lld max_tile_cams=%lld "
                "nnz_blocks=%lld updates=%lld workspace_bytes=%lld sorted_input=%lld\n", (long long)I.E, (long long)I.n_buf, (long long)I.p_tot,
                (long long)I.fixedp, (long long)I.n_all, (long long)I.n, (long long)I.m, (long long)I.pairs, (long long)I.tiles, (long long)I.slots,
                (long long)I.erows, (long long)I.max_tile_cams, (long long)I.nnz_blocks, (long long)I.updates, (long long)I.workspace_bytes,
                (long long)I.sorted_input);
    const PlanDev &d = pl.dev;
    std::printf("  dev");
#define DV(x) std::printf(" " #x "=%lld", (long long)d.x);
    DV(E) DV(n_buf) DV(p_tot) DV(fixedp) DV(n_all) DV(n) DV(D) DV(m) DV(P) DV(T) DV(slots) DV(erows) DV(nnzb) DV(nupd) DV(max_rows16)
    DV(max_tile_pairs) DV(max_tile_slots) DV(max_cams) DV(e_all) DV(sg_n) DV(et_lgts) DV(sp_ok) DV(pm_ok) DV(nlz) DV(dev_id) DV(wide)
    DV(trk_off) DV(em_self) DV(em_ok) DV(em_its) DV(em_lgs) DV(st_ok) DV(st_min) DV(em_min) DV(nlev) DV(ndp) DV(fz_npend) DV(fz_nlazy)
    DV(fz_ok) DV(fzp_ok)
#undef DV
    std::printf("\n  ws");
#define WV(x) std::printf(" " #x "=%zu", pl.ws.x);
    WV(sys) WV(pairacc) WV(zero_bytes) WV(packed) WV(pairgeo) WV(qw) WV(lfac) WV(linv) WV(zvec) WV(dx) WV(dx0) WV(dxg) WV(status) WV(spart)
    WV(esave) WV(total) WV(priv)
#undef WV
    std::printf("\n  plan dev_pm=%d dev_slots=%d dev_wpt=%d dev_q0=%lld dev_f_lo=%lld dev_nw=%lld pm_rounds=%lld k_hi=%lld trk_win_lo=%lld\n", pl.dev_pm,
                pl.dev_slots, pl.dev_wpt, (long long)pl.dev_q0, (long long)pl.dev_f_lo, (long long)pl.dev_nw, pl.pm_rounds, (long long)pl.k_hi,
                (long long)pl.trk_win_lo);
    std::printf("  tables");
#define TV(T, name, solver) dump_vec(#name, pl.name);
    BT_PLAN_TABLES(TV)
#undef TV
    dump_vec("trk_loc", pl.trk_loc); dump_vec("trk_win", pl.trk_win); dump_vec("dev_off", pl.dev_off); dump_vec("dev_pbase", pl.dev_pbase);
    dump_vec("dev_pair_of", pl.dev_pair_of);
    std::printf("\n");
}

// mode 1 .. 4 (above); -100: the mode does not apply to the case
static int build(const Case &c, int mode, bt_plan &pl, Stats &s) {
    pl.recycle();
    if (mode == 4 && c.own_hi <= 0) return -100;
    if (mode >= 3) {
        fill_stats(c, mode == 4, s);
        if (!s.ok) return -100;
        return build_plan_host(nullptr, nullptr, nullptr, c.E, c.n_buf, c.p_tot, c.fixedp, c.n_all_min, c.own_lo, c.own_hi, &pl, nullptr, false, &s.st);
    }
    return build_plan_host(c.ii.data(), c.jj.data(), c.kk.data(), c.E, c.n_buf, c.p_tot, c.fixedp, c.n_all_min, c.own_lo, c.own_hi, &pl, nullptr, mode == 2);
}

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: plan_dump corpus.bin [--time REPEATS]\n"); return 2; }
    const int reps = argc >= 4 && !std::strcmp(argv[2], "--time") ? std::atoi(argv[3]) : 0;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    Case c; bt_plan pl; Stats s;
    for (int idx = 0; read_case(f, c); ++idx) {
        if (reps > 0) {
            for (int mode : {1, 3}) {
                std::vector<double> ms;
                int rc = 0;
                if (mode == 3) { fill_stats(c, false, s); if (!s.ok) continue; }
                for (int r = 0; r < reps; ++r) {
                    pl.recycle();
                    const auto t0 = std::chrono::steady_clock::now();
                    rc = mode == 3 ? build_plan_host(nullptr, nullptr, nullptr, c.E, c.n_buf, c.p_tot, c.fixedp, c.n_all_min, c.own_lo, c.own_hi, &pl, nullptr, false, &s.st)
                                   : build_plan_host(c.ii.data(), c.jj.data(), c.kk.data(), c.E, c.n_buf, c.p_tot, c.fixedp, c.n_all_min, c.own_lo, c.own_hi, &pl);
                    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
                }
                std::sort(ms.begin(), ms.end());
                std::printf("case %d mode %d rc %d median_ms %.3f\n", idx, mode, rc, ms[ms.size() / 2]);
            }
            continue;
        }
        for (int mode = 1; mode <= 4; ++mode) {
            const int rc = build(c, mode, pl, s);
            if (rc == -100) continue;
            std::printf("case %d mode %d rc %d\n", idx, mode, rc);
            if (rc == BT_OK) dump_plan(pl);
        }
    }
    std::fclose(f);
    return 0;
}
