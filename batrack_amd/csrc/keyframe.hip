// keyframe.hip — motion-magnitude keyframe removal and edge pruning for gfx950: the reference's BATRACK.keyframe() /
// keyframe_simple() (main/batrack.py:1011-1073, remove_factors :206-212) as at most six launches that hand their
// results to each other through a status word in device memory.  include/batrack_keyframe.h holds the specification.
//   decide:  k_kf_decide  (grid-stride over the edge list, per-workgroup double partials)  ->  k_kf_finish (one thread adds
//            the partials in index order, takes the means and compares)
//   prune:   k_prune_count (kept edges per tile)  ->  k_prune_scan (one workgroup, exclusive scan in place)  ->
//            k_prune_scatter (predicate recomputed; rank from the wave ballot)
//   shift:   k_rows_shift (a thread owns a column unit of one buffer and walks the rows)
// Ordering comes from the launches only: no workgroup waits on another.  HBM-bound: the index passes read 16 B (decide: jj, and
// ii where jj == k) + 24 B (count) of every edge, the scatter 24 B + the 28 B payload of the kept ones, and writes 52 B per kept edge.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/batrack_ba.h"
#include "../../include/batrack_keyframe.h"
#include "projective_edge.hpp"

namespace bt {

constexpr int KF_THREADS = 256;                 // every kernel here: 4 waves
constexpr int KF_DECIDE_BLOCKS = 256;           // at most this many partials
constexpr int PRUNE_ITERS = 4;                  // 64-edge rows a wave takes
constexpr int PRUNE_WAVE_EDGES = 64 * PRUNE_ITERS;
constexpr int PRUNE_TILE = (KF_THREADS / 64) * PRUNE_WAVE_EDGES;   // 1024 edges per workgroup
constexpr int PRUNE_SCAN_SPAN = KF_THREADS;     // tile counts per pass of the scan

struct DecidePartial { double sum_prev, sum_next; int64_t cnt_prev, cnt_next; };

// workspace: [0, 32) status | [64, 64 + 256*32) decide partials | tile counts / offsets, uint32 per tile
constexpr size_t WS_PARTIALS = 64;
constexpr size_t WS_TILES = WS_PARTIALS + KF_DECIDE_BLOCKS * sizeof(DecidePartial);

static_assert(sizeof(bt_keyframe_status) == 32, "the status word is 32 bytes");

__global__ __launch_bounds__(KF_THREADS) void k_kf_decide(int64_t k, const int64_t *__restrict__ ii, const int64_t *__restrict__ jj,
                                                          const int64_t *__restrict__ kk, int64_t E, const float *__restrict__ poses,
                                                          int64_t n_poses, const float *__restrict__ patches, int64_t n_patches, int pe,
                                                          int cpix, const float *__restrict__ intr, float beta, float one_m_beta,
                                                          DecidePartial *__restrict__ part) {
    double sp = 0.0, sn = 0.0;
    int cp = 0, cn = 0;
    for (int64_t e = (int64_t)blockIdx.x * KF_THREADS + threadIdx.x; e < E; e += (int64_t)gridDim.x * KF_THREADS) {
        const int64_t j = jj[e];
        if (j != k) continue;
        const int64_t i = ii[e];
        const bool prev = i == k - 1;
        if (!prev && i != k + 1) continue;
        const int64_t p = kk[e];
        float f = NAN;
        if (!(i < 0 || j < 0 || p < 0 || i >= n_poses || j >= n_poses || p >= n_patches)) {
            const float *pi = poses + 7 * i, *pj = poses + 7 * j, *Ki = intr + 4 * i, *Kj = intr + 4 * j;
            const float *pat = patches + (size_t)p * 3 * pe + cpix;
            float c0[2], c1[2], c2[2];
            reproject_pixel<false, false>(pi, pi, Ki, Ki, pat, pe, c0);                 // projective_ops.py:115
            reproject_pixel<false, false>(pi, pj, Ki, Kj, pat, pe, c1);                 // :116
            reproject_pixel<false, true>(pi, pj, Ki, Kj, pat, pe, c2);                  // :117
            const float ax = c1[0] - c0[0], ay = c1[1] - c0[1], bx = c2[0] - c0[0], by = c2[1] - c0[1];
            f = beta * sqrtf(ax * ax + ay * ay) + one_m_beta * sqrtf(bx * bx + by * by);   // :119-122
        }
        if (prev) { sp += (double)f; ++cp; } else { sn += (double)f; ++cn; }
    }
    __shared__ double s_p[KF_THREADS], s_n[KF_THREADS];
    __shared__ int c_p[KF_THREADS], c_n[KF_THREADS];
    const int t = threadIdx.x;
    s_p[t] = sp; s_n[t] = sn; c_p[t] = cp; c_n[t] = cn;
    __syncthreads();
    for (int s = KF_THREADS / 2; s > 0; s >>= 1) {                                       // a fixed tree: the same sum every call
        if (t < s) { s_p[t] += s_p[t + s]; s_n[t] += s_n[t + s]; c_p[t] += c_p[t + s]; c_n[t] += c_n[t + s]; }
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = {s_p[0], s_n[0], (int64_t)c_p[0], (int64_t)c_n[0]};
}

__global__ __launch_bounds__(64) void k_kf_finish(const DecidePartial *__restrict__ part, int nparts, double thresh,
                                                  bt_keyframe_status *__restrict__ status) {
    if (threadIdx.x != 0) return;
    double sp = 0.0, sn = 0.0;
    int64_t cp = 0, cn = 0;
    for (int b = 0; b < nparts; ++b) { sp += part[b].sum_prev; sn += part[b].sum_next; cp += part[b].cnt_prev; cn += part[b].cnt_next; }
    const float mp = (float)(sp / (double)cp), mn = (float)(sn / (double)cn);            // 0/0: NaN, torch.mean of nothing
    status->mag_prev = mp;
    status->mag_next = mn;
    status->cnt_prev = (int32_t)cp;
    status->cnt_next = (int32_t)cn;
    status->removed = ((double)mp + (double)mn) / 2.0 < thresh ? 1 : 0;                  // batrack.py:1035-1037; NaN: kept
}

struct PruneArgs {
    int64_t k, M, E;
    int64_t lim0, lim1;        // (n' - removal_window) * M without / with the removal: kk' div M < n' - window  <=>  kk' < lim
};

// the fate of one edge (batrack_keyframe.h (b)); the renumbered indices in i, j, q
__device__ __forceinline__ bool prune_keep(int64_t &i, int64_t &j, int64_t &q, bool r, const PruneArgs &a) {
    if (r) {
        if (i == a.k || j == a.k) return false;
        if (i > a.k) { q -= a.M; i -= 1; }
        if (j > a.k) j -= 1;
        return q >= a.lim1;
    }
    return q >= a.lim0;
}

__device__ __forceinline__ int lanes_below(unsigned long long m) {                       // set bits of m at lanes below this one
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__global__ __launch_bounds__(KF_THREADS) void k_prune_count(const int64_t *__restrict__ ii, const int64_t *__restrict__ jj,
                                                            const int64_t *__restrict__ kk, PruneArgs a,
                                                            const bt_keyframe_status *__restrict__ status, uint32_t *__restrict__ tile_cnt) {
    const bool r = status->removed != 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * PRUNE_TILE + wave * PRUNE_WAVE_EDGES + lane;
    uint32_t cnt = 0;
#pragma unroll
    for (int it = 0; it < PRUNE_ITERS; ++it) {
        const int64_t e = base + it * 64;
        bool keep = false;
        if (e < a.E) {
            int64_t i = ii[e], j = jj[e], q = kk[e];
            keep = prune_keep(i, j, q, r, a);
        }
        cnt += (uint32_t)__popcll(__ballot(keep));
    }
    __shared__ uint32_t wc[KF_THREADS / 64];
    if (lane == 0) wc[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// one workgroup: tile counts -> exclusive offsets, in place, PRUNE_SCAN_SPAN at a time with a carry; the total is E_out
__global__ __launch_bounds__(KF_THREADS) void k_prune_scan(uint32_t *__restrict__ tiles, int64_t ntiles, bt_keyframe_status *__restrict__ status) {
    __shared__ uint32_t s[2][PRUNE_SCAN_SPAN];
    const int t = threadIdx.x;
    uint32_t carry = 0;
    for (int64_t base = 0; base < ntiles; base += PRUNE_SCAN_SPAN) {
        const int64_t idx = base + t;
        const uint32_t v = idx < ntiles ? tiles[idx] : 0u;
        int cur = 0;
        s[0][t] = v;
        __syncthreads();
        for (int d = 1; d < PRUNE_SCAN_SPAN; d <<= 1) {                                  // Hillis-Steele, double-buffered
            s[cur ^ 1][t] = s[cur][t] + (t >= d ? s[cur][t - d] : 0u);
            cur ^= 1;
            __syncthreads();
        }
        if (idx < ntiles) tiles[idx] = carry + s[cur][t] - v;
        carry += s[cur][PRUNE_SCAN_SPAN - 1];
        __syncthreads();                                                                 // s is rewritten by the next pass
    }
    if (t == 0) status->E_out = (int64_t)carry;
}

__global__ __launch_bounds__(KF_THREADS) void k_prune_scatter(const int64_t *__restrict__ ii, const int64_t *__restrict__ jj,
                                                              const int64_t *__restrict__ kk, const float *__restrict__ t3,
                                                              const float *__restrict__ w, const float *__restrict__ wp, PruneArgs a,
                                                              const bt_keyframe_status *__restrict__ status,
                                                              const uint32_t *__restrict__ tile_off, int64_t *__restrict__ ii_o,
                                                              int64_t *__restrict__ jj_o, int64_t *__restrict__ kk_o, float *__restrict__ t3_o,
                                                              float *__restrict__ w_o, float *__restrict__ wp_o) {
    const bool r = status->removed != 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * PRUNE_TILE + wave * PRUNE_WAVE_EDGES + lane;
    int64_t i[PRUNE_ITERS], j[PRUNE_ITERS], q[PRUNE_ITERS];
    unsigned long long b[PRUNE_ITERS];
    bool keep[PRUNE_ITERS];
    uint32_t cnt = 0;
#pragma unroll
    for (int it = 0; it < PRUNE_ITERS; ++it) {
        const int64_t e = base + it * 64;
        keep[it] = false;
        i[it] = j[it] = q[it] = 0;
        if (e < a.E) {
            i[it] = ii[e]; j[it] = jj[e]; q[it] = kk[e];
            keep[it] = prune_keep(i[it], j[it], q[it], r, a);
        }
        b[it] = __ballot(keep[it]);
        cnt += (uint32_t)__popcll(b[it]);
    }
    __shared__ uint32_t wc[KF_THREADS / 64];
    if (lane == 0) wc[wave] = cnt;
    __syncthreads();
    int64_t off = tile_off[blockIdx.x];
    for (int v = 0; v < wave; ++v) off += wc[v];
#pragma unroll
    for (int it = 0; it < PRUNE_ITERS; ++it) {
        if (keep[it]) {
            const int64_t e = base + it * 64, o = off + lanes_below(b[it]);
            ii_o[o] = i[it]; jj_o[o] = j[it]; kk_o[o] = q[it];
            t3_o[3 * o] = t3[3 * e]; t3_o[3 * o + 1] = t3[3 * e + 1]; t3_o[3 * o + 2] = t3[3 * e + 2];
            reinterpret_cast<float2 *>(w_o)[o] = reinterpret_cast<const float2 *>(w)[e];
            reinterpret_cast<float2 *>(wp_o)[o] = reinterpret_cast<const float2 *>(wp)[e];
        }
        off += __popcll(b[it]);
    }
}

struct RowBufs { bt_row_buffer b[BT_KEYFRAME_MAX_BUFFERS]; };

template <typename T>
__device__ __forceinline__ void shift_columns(T *p, int64_t units, int64_t k, int64_t n) {
    for (int64_t c = (int64_t)blockIdx.x * KF_THREADS + threadIdx.x; c < units; c += (int64_t)gridDim.x * KF_THREADS)
        for (int64_t i = k; i < n - 1; ++i) p[i * units + c] = p[(i + 1) * units + c];     // batrack.py:1052-1063
}

__global__ __launch_bounds__(KF_THREADS) void k_rows_shift(RowBufs bufs, int64_t k, int64_t n, const bt_keyframe_status *__restrict__ status) {
    if (status->removed == 0) return;
    void *ptr = bufs.b[blockIdx.y].ptr;
    const int64_t rb = bufs.b[blockIdx.y].row_bytes;
    if ((rb & 3) == 0 && (reinterpret_cast<uintptr_t>(ptr) & 3) == 0) shift_columns(static_cast<uint32_t *>(ptr), rb >> 2, k, n);
    else shift_columns(static_cast<uint8_t *>(ptr), rb, k, n);
}

static bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

static int64_t clamp_i64(__int128 v) {
    const __int128 lo = INT64_MIN, hi = INT64_MAX;
    return (int64_t)(v < lo ? lo : v > hi ? hi : v);
}

static int64_t prune_tiles(int64_t E) { return (E + PRUNE_TILE - 1) / PRUNE_TILE; }

}  // namespace bt

extern "C" size_t bt_keyframe_workspace_bytes(int64_t E) {
    if (E < 0) E = 0;
    return (bt::WS_TILES + (size_t)bt::prune_tiles(E) * sizeof(uint32_t) + 7) & ~(size_t)7;
}
extern "C" int64_t bt_edges_prune_tile(void) { return bt::PRUNE_TILE; }
extern "C" int64_t bt_edges_prune_scan_span(void) { return bt::PRUNE_SCAN_SPAN; }

extern "C" int bt_keyframe_decide(int64_t k, const int64_t *ii, const int64_t *jj, const int64_t *kk, int64_t E, const float *poses,
                                  int64_t n_poses, const float *patches, int64_t n_patches, int64_t patch_elems, const float *intrinsics,
                                  double beta, double thresh, void *workspace, void *stream) {
    if (!workspace || E < 0 || k < -1) return BT_EINVAL;
    if (E > INT32_MAX) return BT_EUNSUPPORTED;
    int nb = 0, p = 0;
    if (k >= 0 && E > 0) {
        if (!ii || !jj || !kk || !poses || !patches || !intrinsics || n_poses < 0 || n_patches < 0 || patch_elems < 1 || patch_elems > 4096)
            return BT_EINVAL;
        while ((int64_t)p * p < patch_elems) ++p;
        if ((int64_t)p * p != patch_elems) return BT_EINVAL;
        const int64_t want = (E + bt::KF_THREADS - 1) / bt::KF_THREADS;
        nb = (int)(want < bt::KF_DECIDE_BLOCKS ? want : bt::KF_DECIDE_BLOCKS);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto *status = static_cast<bt_keyframe_status *>(workspace);
    auto *part = reinterpret_cast<bt::DecidePartial *>(static_cast<char *>(workspace) + bt::WS_PARTIALS);
    if (nb > 0) {
        hipLaunchKernelGGL(bt::k_kf_decide, dim3(nb), dim3(bt::KF_THREADS), 0, st, k, ii, jj, kk, E, poses, n_poses, patches, n_patches,
                           (int)patch_elems, (p / 2) * p + p / 2, intrinsics, (float)beta, (float)(1.0 - beta), part);
        if (hipGetLastError() != hipSuccess) return BT_EHIP;
    }
    hipLaunchKernelGGL(bt::k_kf_finish, dim3(1), dim3(64), 0, st, part, nb, thresh, status);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

extern "C" int bt_edges_prune(int64_t k, int64_t n, int64_t M, int64_t removal_window, const int64_t *ii, const int64_t *jj,
                              const int64_t *kk, const float *targets_3d, const float *weights, const float *weights_pose, int64_t E,
                              int64_t *ii_out, int64_t *jj_out, int64_t *kk_out, float *targets_3d_out, float *weights_out,
                              float *weights_pose_out, void *workspace, void *stream) {
    if (!workspace || E < 0 || M < 1) return BT_EINVAL;
    if (E > INT32_MAX) return BT_EUNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto *status = static_cast<bt_keyframe_status *>(workspace);
    auto *tiles = reinterpret_cast<uint32_t *>(static_cast<char *>(workspace) + bt::WS_TILES);
    const int64_t ntiles = bt::prune_tiles(E);
    if (E > 0) {
        const void *in[6] = {ii, jj, kk, targets_3d, weights, weights_pose};
        void *out[6] = {ii_out, jj_out, kk_out, targets_3d_out, weights_out, weights_pose_out};
        const size_t row[6] = {8, 8, 8, 12, 8, 8};
        for (int a = 0; a < 6; ++a)
            if (!in[a] || !out[a] || ((reinterpret_cast<uintptr_t>(in[a]) | reinterpret_cast<uintptr_t>(out[a])) & (a == 3 ? 3 : 7))) return BT_EINVAL;
        for (int a = 0; a < 6; ++a) {
            const size_t na = row[a] * (size_t)E;
            if (bt::overlap(out[a], na, workspace, bt_keyframe_workspace_bytes(E))) return BT_EINVAL;
            for (int b = 0; b < 6; ++b) {
                if (bt::overlap(out[a], na, in[b], row[b] * (size_t)E)) return BT_EINVAL;
                if (b != a && bt::overlap(out[a], na, out[b], row[b] * (size_t)E)) return BT_EINVAL;
            }
        }
        bt::PruneArgs a;
        a.k = k; a.M = M; a.E = E;
        a.lim0 = bt::clamp_i64(((__int128)n - removal_window) * M);
        a.lim1 = bt::clamp_i64(((__int128)n - 1 - removal_window) * M);
        hipLaunchKernelGGL(bt::k_prune_count, dim3((unsigned)ntiles), dim3(bt::KF_THREADS), 0, st, ii, jj, kk, a, status, tiles);
        if (hipGetLastError() != hipSuccess) return BT_EHIP;
        hipLaunchKernelGGL(bt::k_prune_scan, dim3(1), dim3(bt::KF_THREADS), 0, st, tiles, ntiles, status);
        if (hipGetLastError() != hipSuccess) return BT_EHIP;
        hipLaunchKernelGGL(bt::k_prune_scatter, dim3((unsigned)ntiles), dim3(bt::KF_THREADS), 0, st, ii, jj, kk, targets_3d, weights,
                           weights_pose, a, status, tiles, ii_out, jj_out, kk_out, targets_3d_out, weights_out, weights_pose_out);
    } else {
        hipLaunchKernelGGL(bt::k_prune_scan, dim3(1), dim3(bt::KF_THREADS), 0, st, tiles, (int64_t)0, status);   // E_out = 0
    }
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

extern "C" int bt_rows_shift(const bt_row_buffer *bufs, int32_t nbuf, int64_t k, int64_t n, const void *workspace, void *stream) {
    if (!workspace || nbuf < 0 || nbuf > BT_KEYFRAME_MAX_BUFFERS) return BT_EINVAL;
    if (nbuf == 0) return BT_OK;
    if (!bufs || k < 0 || n < 0) return BT_EINVAL;
    bt::RowBufs rb = {};
    int64_t units = 1;
    for (int b = 0; b < nbuf; ++b) {
        if (!bufs[b].ptr || bufs[b].row_bytes < 1) return BT_EINVAL;
        rb.b[b] = bufs[b];
        const bool words = (bufs[b].row_bytes & 3) == 0 && (reinterpret_cast<uintptr_t>(bufs[b].ptr) & 3) == 0;
        const int64_t u = words ? bufs[b].row_bytes >> 2 : bufs[b].row_bytes;
        if (u > units) units = u;
    }
    if (k >= n - 1) return BT_OK;
    int64_t gx = (units + bt::KF_THREADS - 1) / bt::KF_THREADS;
    if (gx > 2048) gx = 2048;
    hipLaunchKernelGGL(bt::k_rows_shift, dim3((unsigned)gx, (unsigned)nbuf), dim3(bt::KF_THREADS), 0, static_cast<hipStream_t>(stream),
                       rb, k, n, static_cast<const bt_keyframe_status *>(workspace));
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}
