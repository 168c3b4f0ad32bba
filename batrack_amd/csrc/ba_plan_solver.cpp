// ba_plan_solver.cpp — the planner's last phase before the derived tables (ba_plan.cpp): the reduced camera system of a laid-out
// plan — its block pattern, elimination order, symbolic Cholesky factor, level schedule, update triples and the fused
// schedule — or the decision to solve it dense (`wide`).  No HIP calls in this file.
#include "ba_plan.hpp"

#include <algorithm>
#include <numeric>

namespace bt {
namespace {

using Pattern = std::vector<std::vector<uint8_t>>;     // nz[u][v], u >= v: block (u, v) of S may be non-zero

// the cameras of one track (or one tile) couple pairwise
void couple_all(Pattern &nz, std::vector<int32_t> &cset) {
    std::sort(cset.begin(), cset.end());
    cset.erase(std::unique(cset.begin(), cset.end()), cset.end());
    for (size_t u = 0; u < cset.size(); ++u)
        for (size_t v = 0; v <= u; ++v) nz[(size_t)cset[u]][(size_t)cset[v]] = 1;
}

// ---- block structure of S (lower) and symbolic Cholesky ----------------
// S[u][v] (u >= v) may be non-zero if u and v share a tile (Schur term,
// ba.py:321) or form a camera pair with both ends free (B, ba.py:279-282).
int system_pattern(const bt_plan *pl, bool sharded, const DevPlanStats *dstats, const uint64_t *pk, int64_t E, Pattern &nz) {
    const int64_t n = pl->info.n, fixedp = pl->info.fixedp, p_tot = pl->info.p_tot;
    nz.assign((size_t)n, std::vector<uint8_t>((size_t)n, 0));
    for (int64_t c = 0; c < n; ++c) nz[(size_t)c][(size_t)c] = 1;
    // One plan for the whole list: a TILE's cameras couple pairwise — more than its tracks' own couplings where the tracks of a tile
    // see different cameras, and free to have (the tile's product is formed over all of them).  A sharded plan must not: the tiles
    // are this rank's, the pattern is everybody's — there the tracks' own couplings only, of this rank's tracks as of the others'
    // (what a tile adds outside them is a sum of exact zeros: an E row of a camera a track does not see is zero).
    for (int64_t t = 0; t < pl->info.tiles && !sharded; ++t) {
        const int32_t c0 = pl->tile_cam0[(size_t)t], nc = pl->tile_ncam[(size_t)t];
        for (int32_t u = 0; u < nc; ++u)
            for (int32_t v = 0; v <= u; ++v)
                nz[(size_t)pl->tile_cams[(size_t)(c0 + u)]][(size_t)pl->tile_cams[(size_t)(c0 + v)]] = 1;
    }
    for (size_t p = 0; p < pl->pair_i.size(); ++p) {
        const int64_t a = pl->pair_i[p] - fixedp, b = pl->pair_j[p] - fixedp;
        if (a >= 0 && b >= 0) nz[(size_t)std::max(a, b)][(size_t)std::min(a, b)] = 1;
    }
    std::vector<int32_t> cset;
    // a loose track couples all its free cameras (its Schur term, ba.py:321)
    for (size_t l = 0; l < pl->lz_trk.size(); ++l) {
        cset.clear();
        for (int32_t q = pl->lz_ptr[l]; q < pl->lz_ptr[l + 1]; ++q) {
            const int64_t a = pl->pair_i[(size_t)pl->lz_pair[(size_t)q]] - fixedp, b = pl->pair_j[(size_t)pl->lz_pair[(size_t)q]] - fixedp;
            if (a >= 0) cset.push_back((int32_t)a);
            if (b >= 0) cset.push_back((int32_t)b);
        }
        couple_all(nz, cset);
    }
    if (sharded && dstats && dstats->sliced) {
        // (the pattern of the whole list, reduced on the device — k_plan_pattern)
        if (!dstats->pattern) return BT_NEED_EDGES;
        for (int64_t u = 0; u < n; ++u)
            for (int64_t v = 0; v <= u; ++v)
                if ((dstats->pattern[(size_t)u * dstats->pattern_words + (size_t)(v >> 5)] >> (v & 31)) & 1u) nz[(size_t)u][(size_t)v] = 1;
    } else if (sharded && dstats) {
        // (the same from the device's table: a track's cameras are its source frame and the frames of its mask)
        int32_t src_b = -1; uint64_t mask_b = 0, mask2_b = 0;
        for (int64_t p = dstats->kmin; p <= dstats->kmax; ++p) {
            const PatchStat &d = dstats->tab[(size_t)(p - dstats->tab_lo)];
            if (d.cnt <= 0) continue;
            if (d.src == src_b && d.mask == mask_b && d.mask2 == mask2_b) continue;          // (the same cameras as the track before: nothing new)
            src_b = d.src; mask_b = d.mask; mask2_b = d.mask2;
            cset.clear();
            if (d.src >= fixedp) cset.push_back((int32_t)(d.src - fixedp));
            for_targets(d.mask, d.mask2, d.src - 64, [&](int32_t fr) {
                const int64_t c = (int64_t)fr - fixedp;
                if (c >= 0) cset.push_back((int32_t)c);
            });
            couple_all(nz, cset);
        }
    } else if (sharded) {
        // from the edges: all pairs among the free cameras of a track (the camera pair of an edge is among them), every track
        // of the list
        const auto KK = [&](int64_t e) { return (int64_t)(pk[e] >> 32); };
        const auto II = [&](int64_t e) { return (int64_t)((pk[e] >> 16) & 0xffff); };
        const auto JJ = [&](int64_t e) { return (int64_t)(pk[e] & 0xffff); };
        std::vector<int32_t> toff((size_t)p_tot + 1, 0);
        for (int64_t e = 0; e < E; ++e) toff[(size_t)KK(e) + 1]++;
        for (int64_t p = 0; p < p_tot; ++p) toff[(size_t)p + 1] += toff[(size_t)p];
        std::vector<int32_t> tord((size_t)E + 1), tcur(toff.begin(), toff.end() - 1);
        for (int64_t e = 0; e < E; ++e) tord[(size_t)tcur[(size_t)KK(e)]++] = (int32_t)e;
        for (int64_t p = 0; p < p_tot; ++p) {
            if (toff[(size_t)p] == toff[(size_t)p + 1]) continue;
            cset.clear();
            for (int32_t q = toff[(size_t)p]; q < toff[(size_t)p + 1]; ++q) {
                const int32_t e = tord[(size_t)q];
                if (II(e) >= fixedp) cset.push_back((int32_t)(II(e) - fixedp));
                if (JJ(e) >= fixedp) cset.push_back((int32_t)(JJ(e) - fixedp));
            }
            couple_all(nz, cset);
        }
    }
    return BT_OK;
}

// ---- elimination order: two-ended ("twisted") when an index cut gives a small separator
// Cameras are time-ordered and co-visibility is local in time, so a vertex separator is
// looked for as S_k = { j >= k : some i < k is coupled to j }.  Order = [A = {<k} ascending |
// B = {>= k} \ S_k DESCENDING | S_k ascending]: both parts are eliminated from their far end
// towards the separator (no fill beyond their band), their columns are pairwise independent
// and are factored two per level.  Without a useful cut the natural order is kept.
void elimination_order(bt_plan *pl, const Pattern &nz) {
    const int64_t n = pl->info.n;
    std::vector<int32_t> perm((size_t)n);
    std::iota(perm.begin(), perm.end(), 0);
    const int nd = force().natural_order ? 0 : 1;
    int best_k = -1, best_score = (int)n;        // natural chain length = n
    std::vector<uint8_t> in_s((size_t)n);
    for (int64_t k = 1; k < n && nd; ++k) {
        int ns = 0;
        for (int64_t j = k; j < n; ++j) {
            bool coupled = false;
            for (int64_t i = 0; i < k && !coupled; ++i) coupled = nz[(size_t)j][(size_t)i] != 0;
            ns += coupled ? 1 : 0;
        }
        const int na = (int)k, nb = (int)(n - k) - ns;
        if (nb < 1 || ns * 3 > (int)n) continue;
        const int score = std::max(na, nb) + ns;
        if (score < best_score) { best_score = score; best_k = (int)k; }
    }
    if (best_k > 0 && best_score + 2 < (int)n) {
        std::fill(in_s.begin(), in_s.end(), 0);
        for (int64_t j = best_k; j < n; ++j)
            for (int64_t i = 0; i < best_k; ++i) if (nz[(size_t)j][(size_t)i]) { in_s[(size_t)j] = 1; break; }
        size_t o = 0;
        for (int64_t i = 0; i < best_k; ++i) perm[o++] = (int32_t)i;
        for (int64_t j = n - 1; j >= best_k; --j) if (!in_s[(size_t)j]) perm[o++] = (int32_t)j;
        for (int64_t j = best_k; j < n; ++j) if (in_s[(size_t)j]) perm[o++] = (int32_t)j;
    }
    pl->perm = perm;
}

// the factor's block columns in the order of pl->perm (col_ptr, row_idx, blk_col, blk_src) and the elimination tree
int symbolic_factor(bt_plan *pl, const Pattern &nz, std::vector<int32_t> &parent) {
    const int64_t n = pl->info.n;
    const std::vector<int32_t> &perm = pl->perm;
    auto nzp = [&](int64_t a, int64_t b) {            // pattern in the permuted numbering
        const int64_t x = perm[(size_t)a], y = perm[(size_t)b];
        return nz[(size_t)std::max(x, y)][(size_t)std::min(x, y)] != 0;
    };

    // column structures (rows > j), then fill: struct(parent(j)) |= struct(j) \ {parent(j)}
    std::vector<std::vector<int32_t>> cs((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        for (int64_t r = j + 1; r < n; ++r) if (nzp(r, j)) cs[(size_t)j].push_back((int32_t)r);
    }
    parent.assign((size_t)n, -1);
    for (int64_t j = 0; j < n; ++j) {
        auto &sj = cs[(size_t)j];
        std::sort(sj.begin(), sj.end());
        sj.erase(std::unique(sj.begin(), sj.end()), sj.end());
        if (sj.empty()) continue;
        parent[(size_t)j] = sj[0];
        auto &sp = cs[(size_t)sj[0]];
        sp.insert(sp.end(), sj.begin() + 1, sj.end());
    }
    pl->col_ptr.assign((size_t)n + 1, 0);
    pl->row_idx.clear();
    for (int64_t j = 0; j < n; ++j) {
        pl->col_ptr[(size_t)j] = (int32_t)pl->row_idx.size();
        pl->row_idx.push_back((int32_t)j);
        pl->row_idx.insert(pl->row_idx.end(), cs[(size_t)j].begin(), cs[(size_t)j].end());
    }
    pl->col_ptr[(size_t)n] = (int32_t)pl->row_idx.size();
    pl->info.nnz_blocks = (int64_t)pl->row_idx.size();
    if (pl->info.nnz_blocks >= 32768) return BT_EUNSUPPORTED;

    // block -> column map and where each block comes from in the caller-order lower triangle of S:
    // blk_src = (row_nat << 9) | (col_nat << 1) | transposed
    pl->blk_col.assign(pl->row_idx.size(), 0);
    pl->blk_src.assign(pl->row_idx.size(), 0);
    for (int64_t j = 0; j < n; ++j)
        for (int32_t b = pl->col_ptr[(size_t)j]; b < pl->col_ptr[(size_t)j + 1]; ++b) {
            pl->blk_col[(size_t)b] = (int32_t)j;
            const int32_t x = perm[(size_t)pl->row_idx[(size_t)b]], y = perm[(size_t)j];
            pl->blk_src[(size_t)b] = x >= y ? ((x << 9) | (y << 1)) : ((y << 9) | (x << 1) | 1);
        }
    return BT_OK;
}

// ---- level schedule: level(j) = 1 + max level of its children in the elimination tree;
// columns of one level are independent.  At most kMaxLevelCols per level (extra ones move up).
int level_schedule(bt_plan *pl, const std::vector<int32_t> &parent) {
    const int64_t n = pl->info.n;
    std::vector<int32_t> lvl((size_t)n, 0);
    for (int64_t j = 0; j < n; ++j)
        if (parent[(size_t)j] >= 0) lvl[(size_t)parent[(size_t)j]] = std::max(lvl[(size_t)parent[(size_t)j]], lvl[(size_t)j] + 1);
    {
        // enforce the per-level cap, keeping level(parent) > level(child)
        std::vector<int32_t> cnt;
        for (int64_t j = 0; j < n; ++j) {
            int32_t l = lvl[(size_t)j];
            for (;;) {
                if ((size_t)l >= cnt.size()) cnt.resize((size_t)l + 1, 0);
                if (cnt[(size_t)l] < kMaxLevelCols) break;
                ++l;
            }
            cnt[(size_t)l]++;
            lvl[(size_t)j] = l;
            if (parent[(size_t)j] >= 0) lvl[(size_t)parent[(size_t)j]] = std::max(lvl[(size_t)parent[(size_t)j]], l + 1);
        }
    }
    // every column a column updates must sit at a strictly higher level
    for (int64_t j = 0; j < n; ++j)
        for (int32_t b = pl->col_ptr[(size_t)j] + 1; b < pl->col_ptr[(size_t)j + 1]; ++b)
            if (lvl[(size_t)pl->row_idx[(size_t)b]] <= lvl[(size_t)j]) return BT_EINVAL;   // cannot happen: rows are ancestors
    int32_t nlev = 0;
    for (int64_t j = 0; j < n; ++j) nlev = std::max(nlev, lvl[(size_t)j] + 1);
    pl->col_lvl = lvl;
    pl->lvl_ptr.assign((size_t)nlev + 1, 0);
    for (int64_t j = 0; j < n; ++j) pl->lvl_ptr[(size_t)lvl[(size_t)j] + 1]++;
    for (int32_t l = 0; l < nlev; ++l) pl->lvl_ptr[(size_t)l + 1] += pl->lvl_ptr[(size_t)l];
    pl->lvl_cols.assign((size_t)n, 0);
    std::vector<int32_t> cur(pl->lvl_ptr.begin(), pl->lvl_ptr.end() - 1);
    for (int64_t j = 0; j < n; ++j) pl->lvl_cols[(size_t)cur[(size_t)lvl[(size_t)j]]++] = (int32_t)j;
    return BT_OK;
}

// ---- update triples of every column (src1, src2, dst | atomic << 15).  First those whose
// destination is the DIAGONAL block of a column of the next level (that column's critical wave
// applies them itself before factoring: listed per target column in dp), then the rest.
// `atomic` marks a destination that another column of the same level also updates.
void update_triples(bt_plan *pl) {
    const int64_t n = pl->info.n;
    const std::vector<int32_t> &lvl = pl->col_lvl;
    const int32_t nlev = (int32_t)pl->lvl_ptr.size() - 1;
    auto find_pos = [&](int32_t col, int32_t row) {
        const auto b = pl->row_idx.begin() + pl->col_ptr[(size_t)col], e = pl->row_idx.begin() + pl->col_ptr[(size_t)col + 1];
        return (int32_t)(std::lower_bound(b, e, row) - pl->row_idx.begin());
    };
    pl->upd_ptr.assign((size_t)n + 1, 0);
    pl->upd_next.assign((size_t)n + 1, 0);
    pl->upd.clear();
    std::vector<std::vector<int32_t>> dplist((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        pl->upd_ptr[(size_t)j] = (int32_t)(pl->upd.size() / 3);
        const int32_t b = pl->col_ptr[(size_t)j] + 1, e = pl->col_ptr[(size_t)j + 1];
        for (int sub = 0; sub < 2; ++sub)
            for (int32_t s = b; s < e; ++s)
                for (int32_t t2 = b; t2 <= s; ++t2) {
                    const int32_t dcol = pl->row_idx[(size_t)t2];
                    const bool diag_next = s == t2 && lvl[(size_t)dcol] == lvl[(size_t)j] + 1;
                    if (diag_next != (sub == 0)) continue;
                    if (diag_next) { dplist[(size_t)dcol].push_back((int32_t)(pl->upd.size() / 3)); pl->upd_next[(size_t)j]++; }
                    pl->upd.push_back(s); pl->upd.push_back(t2);
                    pl->upd.push_back(find_pos(dcol, pl->row_idx[(size_t)s]));
                }
    }
    pl->upd_ptr[(size_t)n] = (int32_t)(pl->upd.size() / 3);
    pl->info.updates = (int64_t)(pl->upd.size() / 3);
    {
        // shared destinations: scan each level's non-diagonal-next triples
        std::vector<int32_t> seen(pl->row_idx.size(), -1), seen_col(pl->row_idx.size(), -1);
        std::vector<uint8_t> shared(pl->row_idx.size(), 0);
        for (int32_t l = 0; l < nlev; ++l) {
            for (int32_t q = pl->lvl_ptr[(size_t)l]; q < pl->lvl_ptr[(size_t)l + 1]; ++q) {
                const int32_t j = pl->lvl_cols[(size_t)q];
                for (int32_t t = pl->upd_ptr[(size_t)j]; t < pl->upd_ptr[(size_t)j + 1]; ++t) {
                    const int32_t dst = pl->upd[(size_t)t * 3 + 2];
                    if (seen[(size_t)dst] == l && seen_col[(size_t)dst] != j) shared[(size_t)dst] = 1;
                    seen[(size_t)dst] = l; seen_col[(size_t)dst] = j;
                }
            }
            for (int32_t q = pl->lvl_ptr[(size_t)l]; q < pl->lvl_ptr[(size_t)l + 1]; ++q) {
                const int32_t j = pl->lvl_cols[(size_t)q];
                for (int32_t t = pl->upd_ptr[(size_t)j]; t < pl->upd_ptr[(size_t)j + 1]; ++t) {
                    int32_t &dst = pl->upd[(size_t)t * 3 + 2];
                    if (shared[(size_t)(dst & 0x7fff)]) dst |= 0x8000;
                }
            }
            for (int32_t q = pl->lvl_ptr[(size_t)l]; q < pl->lvl_ptr[(size_t)l + 1]; ++q) {
                const int32_t j = pl->lvl_cols[(size_t)q];
                for (int32_t t = pl->upd_ptr[(size_t)j]; t < pl->upd_ptr[(size_t)j + 1]; ++t) shared[(size_t)(pl->upd[(size_t)t * 3 + 2] & 0x7fff)] = 0;
            }
        }
    }
    // y rows updated by more than one column of a level: bit 16 of blk_col marks those blocks
    {
        std::vector<int32_t> seen((size_t)n, -1), cnt((size_t)n, 0);
        for (int32_t l = 0; l < nlev; ++l) {
            for (int pass = 0; pass < 2; ++pass)
                for (int32_t q = pl->lvl_ptr[(size_t)l]; q < pl->lvl_ptr[(size_t)l + 1]; ++q) {
                    const int32_t j = pl->lvl_cols[(size_t)q];
                    for (int32_t b = pl->col_ptr[(size_t)j] + 1; b < pl->col_ptr[(size_t)j + 1]; ++b) {
                        const int32_t r = pl->row_idx[(size_t)b];
                        if (pass == 0) { if (seen[(size_t)r] != l) { seen[(size_t)r] = l; cnt[(size_t)r] = 0; } cnt[(size_t)r]++; }
                        else if (cnt[(size_t)r] > 1) pl->blk_col[(size_t)b] |= 1 << 16;
                    }
                }
        }
    }
    pl->dp_ptr.assign((size_t)n + 1, 0);
    pl->dp.clear();
    for (int64_t j = 0; j < n; ++j) {
        pl->dp_ptr[(size_t)j] = (int32_t)pl->dp.size();
        pl->dp.insert(pl->dp.end(), dplist[(size_t)j].begin(), dplist[(size_t)j].end());
    }
    pl->dp_ptr[(size_t)n] = (int32_t)pl->dp.size();

    pl->lvl_meta.assign((size_t)nlev * kMaxLevelCols * 8, 0);
    for (int32_t l = 0; l < nlev; ++l)
        for (int q = 0; q < kMaxLevelCols; ++q) {
            int32_t *mrow = pl->lvl_meta.data() + ((size_t)l * kMaxLevelCols + q) * 8;
            if (pl->lvl_ptr[(size_t)l] + q >= pl->lvl_ptr[(size_t)l + 1]) { mrow[0] = -1; continue; }
            const int32_t j = pl->lvl_cols[(size_t)pl->lvl_ptr[(size_t)l] + q];
            mrow[0] = j; mrow[1] = pl->col_ptr[(size_t)j]; mrow[2] = pl->col_ptr[(size_t)j + 1] - pl->col_ptr[(size_t)j] - 1;
            mrow[3] = pl->upd_ptr[(size_t)j] + pl->upd_next[(size_t)j];
            mrow[4] = pl->upd_ptr[(size_t)j + 1] - mrow[3];
            mrow[5] = pl->dp_ptr[(size_t)j]; mrow[6] = pl->dp_ptr[(size_t)j + 1] - pl->dp_ptr[(size_t)j];
            mrow[7] = pl->lvl_ptr[(size_t)l + 1] - pl->lvl_ptr[(size_t)l];     // columns in this level
        }
}

// ---- fused schedule (k_solve_fused): ONE phase and one barrier per level.  A column's wave
// applies the updates coming from the level right below to its own diagonal block and panel
// rows itself ("pending": listed per destination block), factors and substitutes; every other
// update ("lazy": destination two or more levels up) runs on the helper waves one level later,
// concurrently with the next level's columns.
//   fz_pend_ptr[nnzb+1], fz_pend[2 k]      (src1, src2) of the pending triples of a block
//   fz_lazy_ptr[n+1],  fz_lazy[3 k]        lazy triples of a column (src1, src2, dst | shared << 15)
//   fz_yurg[nnzb]                          1: the y contribution of this block is pending, not lazy
//   fz_meta[nlev][kMaxLevelCols][8]        col, diag pos, #sub-blocks, first lazy triple, #lazy,
//                                          first wave of the column, #waves (64 panel rows each), #cols
void fused_schedule(bt_plan *pl) {
    const int64_t n = pl->info.n;
    const std::vector<int32_t> &lvl = pl->col_lvl;
    const int32_t nlev = (int32_t)pl->lvl_ptr.size() - 1;
    const size_t nb = pl->row_idx.size();
    std::vector<std::vector<int32_t>> pend(nb);
    pl->fz_lazy_ptr.assign((size_t)n + 1, 0);
    pl->fz_lazy.clear();
    pl->fz_yurg.assign(nb, 0);
    for (int64_t j = 0; j < n; ++j) {
        pl->fz_lazy_ptr[(size_t)j] = (int32_t)(pl->fz_lazy.size() / 3);
        for (int32_t t = pl->upd_ptr[(size_t)j]; t < pl->upd_ptr[(size_t)j + 1]; ++t) {
            const int32_t s1 = pl->upd[(size_t)t * 3], s2 = pl->upd[(size_t)t * 3 + 1], d = pl->upd[(size_t)t * 3 + 2];
            const int32_t dcol = pl->row_idx[(size_t)s2];
            if (lvl[(size_t)dcol] == lvl[(size_t)j] + 1) { pend[(size_t)(d & 0x7fff)].push_back(s1); pend[(size_t)(d & 0x7fff)].push_back(s2); }
            else { pl->fz_lazy.push_back(s1); pl->fz_lazy.push_back(s2); pl->fz_lazy.push_back(d); }
        }
        for (int32_t b = pl->col_ptr[(size_t)j] + 1; b < pl->col_ptr[(size_t)j + 1]; ++b)
            if (lvl[(size_t)pl->row_idx[(size_t)b]] == lvl[(size_t)j] + 1) pl->fz_yurg[(size_t)b] = 1;
    }
    pl->fz_lazy_ptr[(size_t)n] = (int32_t)(pl->fz_lazy.size() / 3);
    pl->fz_pend_ptr.assign(nb + 1, 0);
    pl->fz_pend.clear();
    for (size_t b = 0; b < nb; ++b) {
        pl->fz_pend_ptr[b] = (int32_t)(pl->fz_pend.size() / 2);
        pl->fz_pend.insert(pl->fz_pend.end(), pend[b].begin(), pend[b].end());
    }
    pl->fz_pend_ptr[nb] = (int32_t)(pl->fz_pend.size() / 2);
    // packed per-level record of the (at most two) columns k_solve_fused handles per level, 4 ints each:
    //   [4q]   col | #sub-blocks << 8 | source column of the diagonal block's first pending pair << 16
    //   [4q+1] diag pos | #row waves << 16 | (q = 0: #cols << 24)
    //   [4q+2] first lazy triple | #lazy << 16
    //   [4q+3] source block of the diagonal block's first pending pair | min(#pending, 3) << 15
    pl->fz_pmeta.assign((size_t)nlev * 8, 0);
    for (int32_t l = 0; l < nlev; ++l) {
        const int32_t nc = pl->lvl_ptr[(size_t)l + 1] - pl->lvl_ptr[(size_t)l];
        int32_t *m = pl->fz_pmeta.data() + (size_t)l * 8;
        for (int32_t q = 0; q < nc && q < 2; ++q) {
            const int32_t j = pl->lvl_cols[(size_t)pl->lvl_ptr[(size_t)l] + q];
            const int32_t dpos = pl->col_ptr[(size_t)j], cnt = pl->col_ptr[(size_t)j + 1] - dpos - 1;
            const int32_t k0 = pl->fz_pend_ptr[(size_t)dpos], np = pl->fz_pend_ptr[(size_t)dpos + 1] - k0;
            const int32_t sd = np > 0 ? pl->fz_pend[(size_t)k0 * 2] : 0;
            const int32_t ysrc = np > 0 ? (pl->blk_col[(size_t)sd] & 255) : 0;
            const int32_t lz0 = pl->fz_lazy_ptr[(size_t)j], nlz = pl->fz_lazy_ptr[(size_t)j + 1] - lz0;
            m[4 * q] = j | (cnt << 8) | (ysrc << 16);
            m[4 * q + 1] = dpos | (((6 * cnt + 1 + 63) / 64) << 16);
            m[4 * q + 2] = lz0 | (nlz << 16);
            // which columns (slots) of the level below hold pending sources of this column's blocks: only those
            // have to be waited for by the barrier-free solver (bits 20, 21)
            int32_t dep = 0;
            for (int32_t b = dpos; b < pl->col_ptr[(size_t)j + 1]; ++b)
                for (int32_t k = pl->fz_pend_ptr[(size_t)b]; k < pl->fz_pend_ptr[(size_t)b + 1]; ++k) {
                    const int32_t sc = pl->blk_col[(size_t)pl->fz_pend[(size_t)k * 2]] & 255;
                    for (int32_t q2 = 0; l > 0 && q2 < pl->lvl_ptr[(size_t)l] - pl->lvl_ptr[(size_t)l - 1]; ++q2)
                        if (pl->lvl_cols[(size_t)pl->lvl_ptr[(size_t)l - 1] + q2] == sc) dep |= 1 << q2;
                }
            m[4 * q + 3] = sd | ((np < 3 ? np : 3) << 15) | (dep << 20);
        }
        m[1] |= nc << 24;
    }
    // what the kernel keeps per block, ready-made: row | col << 8 | shared-y << 24 | pending-y << 25, and
    // the first pending pair src1 | src2 << 15 | min(#pending, 3) << 30
    pl->fz_rowinfo.assign(nb, 0);
    pl->fz_pfirst.assign(nb, 0);
    pl->fz_psecond.assign(nb, 0);                       // second pending pair src1 | src2 << 15 (a block gets at most
    bool pend_ok = true;                                //  one from each of the two columns of the level below)
    for (size_t b = 0; b < nb; ++b) {
        pl->fz_rowinfo[b] = pl->row_idx[b] | ((pl->blk_col[b] & 255) << 8) | ((pl->blk_col[b] >> 16) << 24) | (pl->fz_yurg[b] << 25);
        const int32_t k0 = pl->fz_pend_ptr[b], c = pl->fz_pend_ptr[b + 1] - k0;
        if (c > 2) pend_ok = false;
        if (c > 0 && nb < 32768)
            pl->fz_pfirst[b] = (int32_t)((uint32_t)pl->fz_pend[(size_t)k0 * 2] | ((uint32_t)pl->fz_pend[(size_t)k0 * 2 + 1] << 15) |
                                         ((uint32_t)(c < 3 ? c : 3) << 30));
        if (c > 1 && nb < 32768)
            pl->fz_psecond[b] = (int32_t)((uint32_t)pl->fz_pend[(size_t)k0 * 2 + 2] | ((uint32_t)pl->fz_pend[(size_t)k0 * 2 + 3] << 15));
    }
    // back substitution, levels descending, one wave per column slot: a barrier is needed before a level
    // only if one of its columns reads an x_i written by another slot's wave since the last barrier
    pl->bs_sync.assign((size_t)nlev, 0);
    {
        std::vector<int32_t> slot((size_t)n, 0);
        for (int32_t l = 0; l < nlev; ++l)
            for (int32_t qi = pl->lvl_ptr[(size_t)l]; qi < pl->lvl_ptr[(size_t)l + 1]; ++qi)
                slot[(size_t)pl->lvl_cols[(size_t)qi]] = qi - pl->lvl_ptr[(size_t)l];
        int32_t last_barrier = nlev;          // no barrier yet
        for (int32_t l = nlev - 1; l >= 0; --l) {
            bool need = false;
            for (int32_t qi = pl->lvl_ptr[(size_t)l]; qi < pl->lvl_ptr[(size_t)l + 1]; ++qi) {
                const int32_t j = pl->lvl_cols[(size_t)qi];
                for (int32_t b = pl->col_ptr[(size_t)j] + 1; b < pl->col_ptr[(size_t)j + 1]; ++b) {
                    const int32_t i = pl->row_idx[(size_t)b];
                    if (slot[(size_t)i] != slot[(size_t)j] && last_barrier > lvl[(size_t)i] - 1) need = true;
                }
            }
            if (need) { pl->bs_sync[(size_t)l] = 1; last_barrier = l; }
        }
    }
    pl->fz_meta.assign((size_t)nlev * kMaxLevelCols * 8, 0);
    pl->dev.fz_ok = (pl->fz_lazy.size() / 3 < 65536 && pl->row_idx.size() < 32768 && pend_ok) ? 1 : 0;
    pl->dev.fzp_ok = pl->dev.fz_ok;                          // additionally: every column's panel rows (+ y) fit one wave
    for (int64_t j = 0; j < n; ++j) if (6 * (pl->col_ptr[(size_t)j + 1] - pl->col_ptr[(size_t)j] - 1) + 1 > 64) pl->dev.fzp_ok = 0;
    for (int32_t l = 0; l < nlev; ++l) {
        if (pl->lvl_ptr[(size_t)l + 1] - pl->lvl_ptr[(size_t)l] > 2) { pl->dev.fz_ok = 0; pl->dev.fzp_ok = 0; }
        int32_t w0 = 0;
        for (int q = 0; q < kMaxLevelCols; ++q) {
            int32_t *mrow = pl->fz_meta.data() + ((size_t)l * kMaxLevelCols + q) * 8;
            if (pl->lvl_ptr[(size_t)l] + q >= pl->lvl_ptr[(size_t)l + 1]) { mrow[0] = -1; mrow[5] = w0; continue; }
            const int32_t j = pl->lvl_cols[(size_t)pl->lvl_ptr[(size_t)l] + q];
            mrow[0] = j; mrow[1] = pl->col_ptr[(size_t)j]; mrow[2] = pl->col_ptr[(size_t)j + 1] - pl->col_ptr[(size_t)j] - 1;
            mrow[3] = pl->fz_lazy_ptr[(size_t)j]; mrow[4] = pl->fz_lazy_ptr[(size_t)j + 1] - mrow[3];
            mrow[5] = w0; mrow[6] = (6 * mrow[2] + 1 + 63) / 64;
            mrow[7] = pl->lvl_ptr[(size_t)l + 1] - pl->lvl_ptr[(size_t)l];
            w0 += mrow[6];
        }
    }
}

// More than kMaxFree (255) free poses: the block-sparse solvers' tables hold pose numbers in 8 bits and block numbers in 15.
// Such a system (a global / loop-closing adjustment; the reference's dense solve has no size clause, ba.py:60-70) is solved
// DENSE in the global workspace (ba_dense.hip): no symbolic factorisation here, the natural order, every lower block "non-zero".
// The same solver takes the systems of FEWER poses whose block-sparse factor does not fit LDS as double (decided below, once
// the symbolic factorisation has counted its blocks): a hundred poses tied by long-range edges fill in to a nearly dense factor,
// which the block-sparse solvers can only hold as float32 (or in global memory) — 24 ms a solve at 179 poses and a float32
// factor's precision, against the dense solver's 3 ms in double.
#define BT_CLEAR_SOLVER(T, name, solver) if (solver) pl->name.clear();
void go_wide(bt_plan *pl) {
    const int64_t n = pl->info.n;
    pl->dev.wide = 1;
    BT_PLAN_TABLES(BT_CLEAR_SOLVER)
    pl->perm.resize((size_t)n);
    std::iota(pl->perm.begin(), pl->perm.end(), 0);
    pl->col_ptr.assign((size_t)n + 1, 0); pl->upd_ptr.assign((size_t)n + 1, 0); pl->upd_next.assign((size_t)n + 1, 0);
    pl->lvl_ptr.assign(1, 0); pl->dp_ptr.assign((size_t)n + 1, 0);
    pl->dev.fz_ok = 0; pl->dev.fzp_ok = 0;
    pl->info.nnz_blocks = n * (n + 1) / 2; pl->info.updates = 0;
}
#undef BT_CLEAR_SOLVER

}  // namespace

int plan_reduced_system(bt_plan *pl, bool sharded, const DevPlanStats *dstats, const uint64_t *pk, int64_t E, PhaseTimer &tick) {
    const bt_plan_info &I = pl->info;
    const int64_t n = I.n;
    pl->dev.wide = 0;
    if (n > kMaxFree) { go_wide(pl); return BT_OK; }
    {
        Pattern nz;
        std::vector<int32_t> parent;
        int rc = system_pattern(pl, sharded, dstats, pk, E, nz);
        if (rc != BT_OK) return rc;
        tick("9");
        elimination_order(pl, nz);
        if ((rc = symbolic_factor(pl, nz, parent)) != BT_OK) return rc;
        tick("10");
        if ((rc = level_schedule(pl, parent)) != BT_OK) return rc;
    }
    tick("11");
    update_triples(pl);
    tick("12");
    fused_schedule(pl);
    // The factor does not fit LDS as double: float32 with refinement, or the dense solver — whichever is priced lower.  Measured
    // (tools/gpu_solver_choice.py, profiles/r06_solver_choice.txt): a block-sparse solve costs ~2.5 us a level where the float32
    // factor fits LDS, ~8 us from global memory, + 26 ns a block update, and a step takes two of them (three where the first
    // refinement step has not converged) — a 255-pose band of half-width 7: 131 levels, 7k updates, 2.4 ms a step; 255 poses
    // tied by long-range edges: 2.8M updates, 140 ms; the dense solver ~12 us a pose whatever the pattern (255 poses 3.1 ms).
    // Long bands stay block-sparse, filled-in systems go dense (95 poses: 12.4 -> 1.0 ms a step, 255: 211 -> 3.5 ms) and get
    // a float64 factor with it.
    // (a forced solver — tests, measurement — keeps the block-sparse tables whatever their size)
    const size_t nlev = pl->lvl_ptr.size() - 1;
    const auto lds_at = [&](size_t elem) { return solve_lds_bytes_raw((size_t)I.nnz_blocks, (size_t)(6 * n), (size_t)I.updates, (size_t)n, nlev, pl->dp.size(), elem); };
    const double level_us = lds_at(sizeof(float)) <= kLdsBudget ? 2.5 : 8.0;
    if (force().solver < 0 && lds_at(sizeof(double)) > kLdsBudget && 2.2 * (level_us * (double)nlev + 0.026 * (double)I.updates) > 12.0 * (double)n)
        go_wide(pl);
    return BT_OK;
}

}  // namespace bt
