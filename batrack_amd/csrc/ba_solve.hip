// ba_solve.hip — the block-sparse solvers of the reduced camera system (gfx950, wave64; which one: plan_route, ba_step.cpp)
// and the refinement of their float32 factors.  Systems of more than 255 free poses take the dense solver (ba_dense.hip).
#include <hip/hip_runtime.h>

#include "ba_kernels.hpp"
#include "ba_update.hpp"
#include "ba_wave.hpp"

namespace bt {

// ------------------------------------------------------------------ k_solve
// Damped, block-sparse (6x6 blocks) right-looking Cholesky of the reduced camera
// system, with y carried as an extra block row so the forward substitution is
// part of the factorisation.  A <- S + (ep + lm * diag S) I  (ba.py:67); a
// non-positive pivot gives dX = 0 (ba.py:9-13); a NaN in dX retries once with
// lm = 1e-3 (ba.py:324-325).  One workgroup; the factor lives in the workspace.
__device__ inline bool chol6_inv(float *Ablk, float *Linv) {
    // in: lower triangle of a 6x6 block (row-major).  out: L in place, L^-1 in Linv.
    float L[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) L[r][c] = c <= r ? Ablk[6*r + c] : 0.0f;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        float s = L[c][c];
#pragma unroll
        for (int k = 0; k < c; ++k) s -= L[c][k] * L[c][k];
        if (!(s > 0.0f)) ok = false;
        const float l = sqrtf(s), il = 1.0f / l;
        L[c][c] = l;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            float t = L[r][c];
#pragma unroll
            for (int k = 0; k < c; ++k) t -= L[r][k] * L[c][k];
            L[r][c] = t * il;
        }
    }
    float Li[6][6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if (r < c) { Li[r][c] = 0.0f; continue; }
            float t = r == c ? 1.0f : 0.0f;
#pragma unroll
            for (int k = c; k < r; ++k) t -= L[r][k] * Li[k][c];
            Li[r][c] = t / L[r][r];
        }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) { Ablk[6*r + c] = L[r][c]; Linv[6*r + c] = Li[r][c]; }
    return ok;
}

// status word (int index) that k_refine_residual raises when the refinement has converged: the solve behind it returns at once
constexpr int kRefineDone = 210;

__global__ __launch_bounds__(1024) void k_solve_global(PlanDev pd, StepArgs a) {
    if (a.status[kRefineDone] != 0) return;
    __shared__ float part[kMaxFree * 6 + 6];
    __shared__ float tq[6];
    __shared__ int flags[2];          // [0] cholesky failed, [1] NaN in dX
    const int tid = threadIdx.x, nth = blockDim.x;
    const int n = pd.n, D = pd.D;
    float *Lw = a.lfac, *Li = a.linv, *z = a.zvec;
    int status = BT_SOLVE_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const float lm = attempt == 0 ? 1e-4f : 1e-3f;
        if (tid < 2) flags[tid] = 0;
        // load the structurally non-zero blocks of S (+ damping) and y
        for (int idx = tid; idx < pd.nnzb * 36; idx += nth) {
            const int b = idx / 36, e = idx % 36, r = e / 6, c = e % 6;
            const int row = pd.row_idx[b], col = pd.blk_col[b] & 255, src = pd.blk_src[b];
            const int rn = src >> 9, cn = (src >> 1) & 255;
            const int rr = (src & 1) ? c : r, cc = (src & 1) ? r : c;       // transposed source block
            double v = (row > col || r >= c) ? a.S[(size_t)(6*rn + rr) * D + 6*cn + cc] : 0.0;
            if (row == col && r == c) v = v + ((double)a.ep + (double)lm * v);
            Lw[idx] = (float)v;
        }
        for (int i = tid; i < D; i += nth) z[i] = (float)a.y[6 * pd.perm[i / 6] + i % 6];
        __syncthreads();

        for (int j = 0; j < n; ++j) {
            const int dpos = pd.col_ptr[j], cnt = pd.col_ptr[j + 1] - dpos - 1;
            if (tid == 0) {
                if (!chol6_inv(Lw + (size_t)dpos * 36, Li + (size_t)j * 36)) flags[0] = 1;
                float zz[6];
                for (int r = 0; r < 6; ++r) {                       // z_j <- L_jj^-1 z_j
                    float t = 0.0f;
                    for (int c = 0; c <= r; ++c) t += Li[j*36 + 6*r + c] * z[6*j + c];
                    zz[r] = t;
                }
                for (int r = 0; r < 6; ++r) z[6*j + r] = zz[r];
            }
            __syncthreads();
            // L_ij = A_ij L_jj^-T, one thread per block row; then y_i -= L_ij z_j
            for (int idx = tid; idx < cnt * 6; idx += nth) {
                const int s = idx / 6, r = idx % 6;
                float *blk = Lw + (size_t)(dpos + 1 + s) * 36 + 6*r;
                float in[6], out[6];
                for (int c = 0; c < 6; ++c) in[c] = blk[c];
                float dot = 0.0f;
                for (int c = 0; c < 6; ++c) {
                    float t = 0.0f;
                    for (int k = 0; k <= c; ++k) t += in[k] * Li[j*36 + 6*c + k];
                    out[c] = t;
                    dot += t * z[6*j + c];
                }
                for (int c = 0; c < 6; ++c) blk[c] = out[c];
                z[6 * pd.row_idx[dpos + 1 + s] + r] -= dot;
            }
            __syncthreads();
            const int u0 = pd.upd_ptr[j], nu = pd.upd_ptr[j + 1] - u0;
            for (int idx = tid; idx < nu * 36; idx += nth) {
                const int t = idx / 36, e = idx % 36, r = e / 6, c = e % 6;
                const int *tr = pd.upd + (size_t)(u0 + t) * 3;
                const float *L1 = Lw + (size_t)tr[0] * 36 + 6*r, *L2 = Lw + (size_t)tr[1] * 36 + 6*c;
                float acc = 0.0f;
                for (int k = 0; k < 6; ++k) acc += L1[k] * L2[k];
                Lw[(size_t)(tr[2] & 0x7fff) * 36 + e] -= acc;
            }
            __syncthreads();
        }

        // back substitution x = L^-T z, in place in z
        for (int j = n - 1; j >= 0; --j) {
            const int dpos = pd.col_ptr[j], cnt = pd.col_ptr[j + 1] - dpos - 1;
            for (int idx = tid; idx < cnt * 6; idx += nth) {
                const int s = idx / 6, c = idx % 6;
                const float *blk = Lw + (size_t)(dpos + 1 + s) * 36;
                const float *xr = z + 6 * pd.row_idx[dpos + 1 + s];
                float t = 0.0f;
                for (int r = 0; r < 6; ++r) t += blk[6*r + c] * xr[r];
                part[idx] = t;
            }
            __syncthreads();
            if (tid < 6) {
                float t = z[6*j + tid];
                for (int s = 0; s < cnt; ++s) t -= part[6*s + tid];
                tq[tid] = t;
            }
            __syncthreads();
            if (tid < 6) {
                float x = 0.0f;
                for (int r = tid; r < 6; ++r) x += Li[j*36 + 6*r + tid] * tq[r];
                z[6*j + tid] = x;
            }
            __syncthreads();
        }
        for (int i = tid; i < D; i += nth) if (z[i] != z[i]) flags[1] = 1;
        __syncthreads();
        const bool failed = flags[0] != 0, has_nan = flags[1] != 0;
        __syncthreads();
        if (failed) {                                   // zeros, and zeros hold no NaN: done
            for (int i = tid; i < D; i += nth) z[i] = 0.0f;
            status = BT_SOLVE_CHOL_FAILED;
            break;
        }
        if (!has_nan) break;
        status = BT_SOLVE_RETRIED;
    }
    __syncthreads();
    for (int i = tid; i < D; i += nth) a.dx[6 * pd.perm[i / 6] + i % 6] = z[i];
    if (tid == 0) a.status[0] = status;
}

// ------------------------------------------------------------------ k_solve_lds
// The same factorisation with the factor resident in LDS.  A lone wave retires
// roughly one instruction per 6-10 cycles on this part, so the sweep is written
// for the fewest instructions on the critical path, two short phases per column:
//   phase 1   wave 0: apply column j-1's update to the diagonal block of column j,
//             factor it (every lane redundantly, in registers), store L_jj;
//             all other waves: every other update of column j-1 (into column j's
//             sub-diagonal blocks, into later columns, and into y)
//   phase 2   all threads: one block row each of L_ij = A_ij L_jj^-T by forward
//             substitution; the extra row is y_j (forward substitution of the RHS)
// The diagonal block keeps L_jj with 1/l_cc on its diagonal.  After the sweep all
// threads bring the factor into back-substitution form (M_ij = (L_ij L_jj^-1)^T:
// lds_backsub_prep), and wave 0 runs the sequential back substitution with DPP reductions.
#define BT_LT(r, c) ((r) * ((r) + 1) / 2 + (c))

// in place: lower triangle (packed) -> its Cholesky factor, diagonal entries hold 1 / l_cc.
template <typename T>
__device__ __forceinline__ bool chol6_packed(T (&L)[21]) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        T s = L[BT_LT(c, c)];
#pragma unroll
        for (int k = 0; k < c; ++k) s -= L[BT_LT(c, k)] * L[BT_LT(c, k)];
        ok = ok && (s > (T)0);
        const T il = rsqrt_t<T>(s);
        L[BT_LT(c, c)] = il;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            T t = L[BT_LT(r, c)];
#pragma unroll
            for (int k = 0; k < c; ++k) t -= L[BT_LT(r, k)] * L[BT_LT(c, k)];
            L[BT_LT(r, c)] = t * il;
        }
    }
    return ok;
}

// The factor into back-substitution form, in one pass with one thread per factor block: M_ij = (L_ij L_jj^-1)^T in place
// of L_ij, i.e. Mt[r][c] = sum_{k>=c} Linv_j[k][c] L_ij[r][k], and zt_j[c] = sum_{k>=c} Linv_j[k][c] z_j[k] from the thread
// of the diagonal block.  Every thread reads its column's diagonal block (the lanes of a column the same addresses: a
// broadcast), factors it where the sweep left the updated A_jj there (RAW_DIAG; otherwise it holds L_jj with 1/l_cc on the
// diagonal) and inverts it in registers - redundantly, which costs the dependent chain once whether 63 threads or 476 walk
// it - and transforms its own six rows.  L_jj^-1 is stored nowhere: the level loop reads off-diagonal M entries and zt only,
// a retry loads the whole factor again.  Race-free by construction: an off-diagonal block is read and written by its own
// thread alone, diagonal blocks and z are only read, zt_j is written by one thread; no barrier inside.
// `row_idx`: row | col << 8 per block; the diagonal block of column j is block col_ptr[j].
template <typename T, bool RAW_DIAG>
__device__ __forceinline__ void lds_backsub_prep(T *Lw, const T *z, T *zt, const int *row_idx, const int *col_ptr, int nnzb, int tid, int nth) {
    for (int b = tid; b < nnzb; b += nth) {
        const int rc = row_idx[b], j = (rc >> 8) & 255;
        const bool diag = (rc & 255) == j;
        const T *dblk = Lw + (size_t)col_ptr[j] * 36;
        T L[21], li[21];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            T row[6];
            load_row6(dblk + 6 * r, row);
#pragma unroll
            for (int c = 0; c <= r; ++c) L[BT_LT(r, c)] = row[c];
        }
        if (RAW_DIAG) (void)chol6_packed<T>(L);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            li[BT_LT(c, c)] = L[BT_LT(c, c)];
#pragma unroll
            for (int r = c + 1; r < 6; ++r) {
                T t = (T)0;
#pragma unroll
                for (int k = c; k < r; ++k) t += L[BT_LT(r, k)] * li[BT_LT(k, c)];
                li[BT_LT(r, c)] = -t * L[BT_LT(r, r)];
            }
        }
        auto to_m = [&](const T (&in)[6], T (&out)[6]) {
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                T t = li[BT_LT(c, c)] * in[c];
#pragma unroll
                for (int k = c + 1; k < 6; ++k) t += li[BT_LT(k, c)] * in[k];
                out[c] = t;
            }
        };
        if (diag) {
            T in[6], out[6];
            load_row6(z + 6 * j, in);
            to_m(in, out);
            store_row6(zt + 6 * j, out);
        } else {
            // rows two at a time: their loads in flight together, and no more than 12 values beside li (three at a time
            // cost k_solve_lds<double> two registers)
            T *p = Lw + (size_t)b * 36;
            for (int h = 0; h < 3; ++h, p += 12) {
                T in[2][6], out[2][6];
#pragma unroll
                for (int u = 0; u < 2; ++u) load_row6(p + 6 * u, in[u]);
#pragma unroll
                for (int u = 0; u < 2; ++u) to_m(in[u], out[u]);
#pragma unroll
                for (int u = 0; u < 2; ++u) store_row6(p + 6 * u, out[u]);
            }
        }
    }
}

size_t solve_lds_bytes(const PlanDev &pd, size_t elem) {
    return solve_lds_bytes_raw((size_t)pd.nnzb, (size_t)pd.D, (size_t)pd.nupd, (size_t)pd.n, (size_t)pd.nlev, (size_t)pd.ndp, elem);
}

template <typename T> __device__ __forceinline__ void lds_sub(T *p, T v, bool atomic) {
    if (atomic) atomicAdd(p, -v); else *p -= v;
}

// One ROW of an update triple: dst[r][:] -= (row r of block tr[0]) . (rows of block tr[1])^T.
// 21 vector LDS loads and 36 FMAs for 6 outputs.  Bit 15 of tr[2]: the destination is also
// updated by another column of the same level -> LDS atomics.
// (the triple as three values: callers that keep it packed in one 8-byte LDS word)
template <typename T>
__device__ __forceinline__ void apply_update_row3(T *Lw, unsigned s1, unsigned s2, unsigned d, int r) {
    T a[6], b[36], o[6], v[6];
    T *dst = Lw + (d & 0x7fffu) * 36 + 6 * r;
    const T *bb = Lw + s2 * 36;
    load_row6(Lw + s1 * 36 + 6 * r, a);
#pragma unroll
    for (int c = 0; c < 6; ++c) load_row6(bb + 6 * c, reinterpret_cast<T (&)[6]>(b[6 * c]));
    load_row6(dst, v);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        T acc = a[0] * b[6 * c];
#pragma unroll
        for (int k = 1; k < 6; ++k) acc += a[k] * b[6 * c + k];
        o[c] = acc;
    }
    if (d & 0x8000u) {
#pragma unroll
        for (int c = 0; c < 6; ++c) atomicAdd(dst + c, -o[c]);
    } else {
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] -= o[c];
        store_row6(dst, v);
    }
}

template <typename T, bool PROF = false>
__device__ __forceinline__ void apply_update_row(T *Lw, const unsigned short *tr, int r, long long *pf = nullptr, long long *tcp = nullptr) {
    T a[6], b[36], o[6], v[6];
    const unsigned d = tr[2];
    if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long tn = clock64(); pf[2] += tn - *tcp; *tcp = tn; }
    T *dst = Lw + (size_t)(d & 0x7fffu) * 36 + 6 * r;
    const T *bb = Lw + (size_t)tr[1] * 36;
    // all 24 vector loads are issued before any arithmetic: one LDS latency instead of one per row
    load_row6(Lw + (size_t)tr[0] * 36 + 6 * r, a);
#pragma unroll
    for (int c = 0; c < 6; ++c) load_row6(bb + 6 * c, reinterpret_cast<T (&)[6]>(b[6 * c]));
    load_row6(dst, v);
    __builtin_amdgcn_sched_barrier(0);
    if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long tn = clock64(); pf[4] += tn - *tcp; *tcp = tn; }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        T acc = a[0] * b[6 * c];
#pragma unroll
        for (int k = 1; k < 6; ++k) acc += a[k] * b[6 * c + k];
        o[c] = acc;
    }
    if (d & 0x8000u) {
#pragma unroll
        for (int c = 0; c < 6; ++c) atomicAdd(dst + c, -o[c]);
    } else {
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] -= o[c];
        store_row6(dst, v);
    }
    if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long tn = clock64(); pf[9] += tn - *tcp; *tcp = tn; }
}

// (the three LDS solvers are device functions so that the fused solve + update launch can run them in its first workgroup —
//  ba_solve_update.hpp; PUB: dX also goes out as tagged granules, at the one point where it is final.  The kernels follow each.)
template <typename T, bool PROF, bool PUB>
__device__ __forceinline__ void solve_lds_body(const PlanDev &pd, const StepArgs &a) {
    if (sizeof(T) == 4 && a.status[kRefineDone] != 0) return;       // (the double factor solves once: no refinement, no flag)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int flags[2];
    const int tid = threadIdx.x, nth = blockDim.x, wave = tid >> 6, lane = tid & 63;
    const int n = pd.n, D = pd.D, nnzb = pd.nnzb, nlev = pd.nlev;
    T *Lw = reinterpret_cast<T *>(smem);
    T *z = Lw + (size_t)nnzb * 36, *zt = z + D;
    size_t off = (((size_t)nnzb * 36 + 2 * (size_t)D) * sizeof(T) + 15) / 16 * 16;
    unsigned short *upd = reinterpret_cast<unsigned short *>(smem + off);
    off = (off + (size_t)pd.nupd * 3 * sizeof(unsigned short) + 15) / 16 * 16;
    int *row_idx = reinterpret_cast<int *>(smem + off), *col_ptr = row_idx + nnzb, *upd_ptr = col_ptr + n + 1,
        *upd_next = upd_ptr + n + 1, *dp_ptr = upd_next + n + 1, *lvl_ptr = dp_ptr + n + 1,
        *lvl_cols = lvl_ptr + nlev + 1, *dp = lvl_cols + n;
    int4 *lvl_meta = reinterpret_cast<int4 *>(smem + ((reinterpret_cast<unsigned char *>(dp + pd.ndp) - smem + 15) / 16 * 16));
    long long pf[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tc = PROF ? clock64() : 0, tn;
#define BT_PF(i) do { if (PROF) { tn = clock64(); pf[i] += tn - tc; tc = tn; } } while (0)
    for (int i = tid; i < pd.nupd * 3; i += nth) upd[i] = (unsigned short)pd.upd[i];
    for (int i = tid; i < nnzb; i += nth) row_idx[i] = pd.row_idx[i] | (pd.blk_col[i] << 8);   // row | col << 8 | shared-y << 24
    for (int i = tid; i <= n; i += nth) {
        col_ptr[i] = pd.col_ptr[i]; upd_ptr[i] = pd.upd_ptr[i]; upd_next[i] = pd.upd_next[i]; dp_ptr[i] = pd.dp_ptr[i];
    }
    for (int i = tid; i <= nlev; i += nth) lvl_ptr[i] = pd.lvl_ptr[i];
    for (int i = tid; i < n; i += nth) lvl_cols[i] = pd.lvl_cols[i];
    for (int i = tid; i < pd.ndp; i += nth) dp[i] = pd.dp[i];
    for (int i = tid; i < nlev * kMaxLevelCols * 2; i += nth) lvl_meta[i] = reinterpret_cast<const int4 *>(pd.lvl_meta)[i];
    __syncthreads();

    int status = BT_SOLVE_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const double lm = attempt == 0 ? 1e-4 : 1e-3;
        if (tid < 2) flags[tid] = 0;
        // one thread per block row: 6 doubles of S (caller order, lower triangle; blk_src says where
        // and whether transposed); 4 rounds of loads in flight
        for (int base = 0; base < nnzb * 6; base += 2 * nth) {
            double v[2][6];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int idx = base + u * nth + tid;
                if (idx < nnzb * 6) {
                    const int b = idx / 6, r = idx - 6 * b, src = pd.blk_src[b];
                    const int rn = src >> 9, cn = (src >> 1) & 255;
                    if (src & 1) {
#pragma unroll
                        for (int c = 0; c < 6; ++c) v[u][c] = a.S[(size_t)(6 * rn + c) * D + 6 * cn + r];
                    } else {
                        const double *p = a.S + (size_t)(6 * rn + r) * D + 6 * cn;
#pragma unroll
                        for (int c = 0; c < 6; ++c) v[u][c] = p[c];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int idx = base + u * nth + tid;
                if (idx < nnzb * 6) {
                    const int b = idx / 6, r = idx - 6 * b, rc = row_idx[b];
                    const bool diag = (rc & 255) == ((rc >> 8) & 255);
                    T w[6];
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
                        double x = (!diag || r >= c) ? v[u][c] : 0.0;
                        if (diag && r == c) x = x + ((double)a.ep + lm * x);          // ba.py:67
                        w[c] = (T)x;
                    }
                    store_row6(Lw + (size_t)b * 36 + 6 * r, w);
                }
            }
        }
        for (int i = tid; i < D; i += nth) z[i] = (T)a.y[6 * pd.perm[i / 6] + i % 6];
        __syncthreads();
        BT_PF(0);

        // Per-level metadata (wave-uniform, kept in SGPRs).  The entry of level l+1 is fetched from LDS
        // before the barrier that ends level l, so its latency hides behind the barrier.
        int4 cA0, cA1, cA2, cA3, pA0, pA1, pA2, pA3, cW, cWb;     // current / previous level, and this wave's own column
        int cn0, cn1, cn2, cn3, pn0 = 0, pn1 = 0, pn2 = 0, pn3 = 0, nc;
        pA0 = pA1 = pA2 = pA3 = make_int4(-1, 0, 0, 0);
        auto fetch_level = [&](int l) {
            const int4 *ml = lvl_meta + (size_t)l * kMaxLevelCols * 2;
            cA0 = uniform4(ml[0]); cA1 = uniform4(ml[2]); cA2 = uniform4(ml[4]); cA3 = uniform4(ml[6]);
            const int4 b0 = uniform4(ml[1]);
            cn0 = b0.x; nc = b0.w;
            cn1 = __builtin_amdgcn_readfirstlane(ml[3].x); cn2 = __builtin_amdgcn_readfirstlane(ml[5].x);
            cn3 = __builtin_amdgcn_readfirstlane(ml[7].x);
            const int wq = wave < kMaxLevelCols ? wave : 0;
            cW = uniform4(ml[2 * wq]); cWb = uniform4(ml[2 * wq + 1]);
        };
        fetch_level(0);
        long long ph1 = 0, ph2 = 0, tph = PROF ? clock64() : 0;
        for (int l = 0; l < nlev; ++l) {
            if (PROF) tph = clock64();
            // ---- phase 1
            if (wave < nc) {
                __builtin_amdgcn_s_setprio(3);            // the critical path of the level: win issue arbitration on this SIMD
                const int4 ma = cW, mb = cWb;
                const int dpos = ma.y;
                for (int k = mb.y; k < mb.y + mb.z; ++k) {        // pending updates of this column's diagonal block
                    if (lane < 36) {
                        const unsigned short *tr = upd + 3 * dp[k];
                        const int r = lane / 6, c = lane - 6 * r;
                        const T *src = Lw + (size_t)tr[0] * 36;
                        T x[6], y[6];
                        load_row6(src + 6 * r, x);
                        load_row6(src + 6 * c, y);
                        T acc = x[0] * y[0];
#pragma unroll
                        for (int q = 1; q < 6; ++q) acc += x[q] * y[q];
                        Lw[(size_t)dpos * 36 + lane] -= acc;
                    }
                    wave_fence();
                }
                T L[21];
                const T *dblk = Lw + (size_t)dpos * 36;
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    T row[6];
                    load_row6(dblk + 6 * r, row);
#pragma unroll
                    for (int c = 0; c <= r; ++c) L[BT_LT(r, c)] = row[c];
                }
                const bool ok = chol6_packed<T>(L);
                BT_PF(2);
                if (lane == 0) {                 // entries above the diagonal are don't-care: nothing reads them
                    if (!ok) flags[0] = 1;
#pragma unroll
                    for (int r = 0; r < 6; ++r) {
                        T row[6];
#pragma unroll
                        for (int c = 0; c < 6; ++c) row[c] = L[BT_LT(r, c <= r ? c : r)];
                        store_row6(Lw + (size_t)dpos * 36 + 6 * r, row);
                    }
                }
                BT_PF(4);
                __builtin_amdgcn_s_setprio(0);
            } else if (l > 0) {
                // the other update triples of the previous level's columns (one ROW of a triple per
                // thread) and their contribution to y, all columns flattened over the helper threads
                const int h = tid - 64 * nc, hs = nth - 64 * nc;
                const int nu0 = pn0, nu1 = pn1, nu2 = pn2, nu3 = pn3;
                // (a) update rows of all columns of the previous level, flattened over the helper threads
                int rows_b[kMaxLevelCols + 1];
                rows_b[0] = 0;
                rows_b[1] = pA0.x >= 0 ? nu0 * 6 : 0;
                rows_b[2] = rows_b[1] + (pA1.x >= 0 ? nu1 * 6 : 0);
                rows_b[3] = rows_b[2] + (pA2.x >= 0 ? nu2 * 6 : 0);
                rows_b[4] = rows_b[3] + (pA3.x >= 0 ? nu3 * 6 : 0);
                BT_PF(0);                 // (helper waves: slot 0 = time from the barrier to the first item)
                for (int item = h; item < rows_b[kMaxLevelCols]; item += hs) {
                    int q = 0;
#pragma unroll
                    for (int k = 1; k < kMaxLevelCols; ++k) q += item >= rows_b[k] ? 1 : 0;
                    const int idx = item - (q == 0 ? 0 : q == 1 ? rows_b[1] : q == 2 ? rows_b[2] : rows_b[3]);
                    const int4 pa = q == 0 ? pA0 : q == 1 ? pA1 : q == 2 ? pA2 : pA3;
                    const int t = idx / 6;
                    apply_update_row<T, PROF>(Lw, upd + 3 * (pa.w + t), idx - 6 * t, pf, &tc);
                }
                // (b) their contribution to y, on the waves after those that had update rows (no wave
                //     runs both kinds of item in the common one-round case)
                int ys_b[kMaxLevelCols + 1];
                ys_b[0] = 0;
                ys_b[1] = pA0.x >= 0 ? pA0.z * 6 : 0;
                ys_b[2] = ys_b[1] + (pA1.x >= 0 ? pA1.z * 6 : 0);
                ys_b[3] = ys_b[2] + (pA2.x >= 0 ? pA2.z * 6 : 0);
                ys_b[4] = ys_b[3] + (pA3.x >= 0 ? pA3.z * 6 : 0);
                const int shift = ((rows_b[kMaxLevelCols] + 63) >> 6) << 6;
                for (int item = (h - shift % hs + hs) % hs; item < ys_b[kMaxLevelCols]; item += hs) {
                    int q = 0;
#pragma unroll
                    for (int k = 1; k < kMaxLevelCols; ++k) q += item >= ys_b[k] ? 1 : 0;
                    const int qq = item - (q == 0 ? 0 : q == 1 ? ys_b[1] : q == 2 ? ys_b[2] : ys_b[3]);
                    const int4 pa = q == 0 ? pA0 : q == 1 ? pA1 : q == 2 ? pA2 : pA3;
                    const int pj = pa.x, dposp = pa.y, sb = qq / 6, r = qq - 6 * sb;
                    T lr[6], zr[6];
                    load_row6(Lw + (size_t)(dposp + 1 + sb) * 36 + 6 * r, lr);
                    load_row6(z + 6 * pj, zr);
                    T acc = lr[0] * zr[0];
#pragma unroll
                    for (int k = 1; k < 6; ++k) acc += lr[k] * zr[k];
                    const int rcv = row_idx[dposp + 1 + sb];
                    lds_sub(z + 6 * (rcv & 255) + r, acc, (rcv >> 24) != 0);
                }
                BT_PF(1);
            }
            if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); ph1 += clock64() - tph; }
            __syncthreads();
            if (PROF) tph = clock64();
            BT_PF(5);
            // ---- phase 2: block rows of the level's columns (and their y) by forward substitution
            {
                const int4 mA0 = cA0, mA1 = cA1, mA2 = cA2, mA3 = cA3;
                int rows_before[kMaxLevelCols + 1];
                rows_before[0] = 0;
                rows_before[1] = mA0.x >= 0 ? mA0.z * 6 + 1 : 0;
                rows_before[2] = rows_before[1] + (mA1.x >= 0 ? mA1.z * 6 + 1 : 0);
                rows_before[3] = rows_before[2] + (mA2.x >= 0 ? mA2.z * 6 + 1 : 0);
                rows_before[4] = rows_before[3] + (mA3.x >= 0 ? mA3.z * 6 + 1 : 0);
                for (int item = tid; item < rows_before[kMaxLevelCols]; item += nth) {
                    int q = 0;
#pragma unroll
                    for (int k = 1; k < kMaxLevelCols; ++k) q += item >= rows_before[k] ? 1 : 0;
                    const int rw = item - (q == 0 ? 0 : q == 1 ? rows_before[1] : q == 2 ? rows_before[2] : rows_before[3]);
                    const int4 ma = q == 0 ? mA0 : q == 1 ? mA1 : q == 2 ? mA2 : mA3;
                    const int j = ma.x, dpos = ma.y, cnt = ma.z;
                    T L[21];
                    const T *dblk = Lw + (size_t)dpos * 36;
#pragma unroll
                    for (int r = 0; r < 6; ++r) {
                        T row[6];
                        load_row6(dblk + 6 * r, row);
#pragma unroll
                        for (int c = 0; c <= r; ++c) L[BT_LT(r, c)] = row[c];
                    }
                    T *p = rw < cnt * 6 ? Lw + (size_t)(dpos + 1) * 36 + 6 * rw : z + 6 * j;
                    T in[6], out[6];
                    load_row6(p, in);
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
                        T t = in[c];
#pragma unroll
                        for (int k = 0; k < c; ++k) t -= out[k] * L[BT_LT(c, k)];
                        out[c] = t * L[BT_LT(c, c)];
                    }
                    store_row6(p, out);
                }
            }
            BT_PF(3);
            if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); ph2 += clock64() - tph; }
            pA0 = cA0; pA1 = cA1; pA2 = cA2; pA3 = cA3; pn0 = cn0; pn1 = cn1; pn2 = cn2; pn3 = cn3;
            if (l + 1 < nlev) fetch_level(l + 1);
            __syncthreads();
            BT_PF(5);
        }

        if (PROF && lane == 0) {
            long long *o = reinterpret_cast<long long *>(a.status + 4) + 40 + wave * 2;
            o[0] = ph1; o[1] = ph2;
        }
        // ---- back-substitution form (M_ij in place of L_ij, zt from z), one thread per factor block
        lds_backsub_prep<T, false>(Lw, z, zt, row_idx, col_ptr, nnzb, tid, nth);
        __syncthreads();
        BT_PF(6);
        // (c) x_j = zt_j - sum_{i>j} M_ij x_i, levels descending; one wave per column of the level,
        //     lane = (component c) * 8 + g
        for (int l = nlev - 1; l >= 0; --l) {
            const int4 ma = uniform4(lvl_meta[(l * kMaxLevelCols + (wave < kMaxLevelCols ? wave : 0)) * 2]);
            if (wave < kMaxLevelCols && ma.x >= 0) {
                const int c = lane >> 3, g = lane & 7;
                const int j = ma.x, dpos = ma.y, cnt = ma.z;
                T acc = (T)0;
                if (c < 6)
                    for (int sb = g; sb < cnt; sb += 8) {           // one sub-block per lane group
                        const int b = dpos + 1 + sb;
                        T x[6];
                        load_row6(zt + 6 * (row_idx[b] & 255), x);
                        const T *mb = Lw + (size_t)b * 36 + c;     // Mt[r][c]
                        acc += mb[0] * x[0] + mb[6] * x[1] + mb[12] * x[2] + mb[18] * x[3] + mb[24] * x[4] + mb[30] * x[5];
                    }
                acc = dpp_add8(acc);
                if (c < 6 && g == 0) zt[6 * j + c] -= acc;
            }
            __syncthreads();
        }
        BT_PF(7);
        // (this epilogue also ends k_solve_fused and k_solve_pipe: as one function the branch that ends an attempt came out inverted in all three;
        //  not measured on the GPU, so it stays three times -- profiles/r15_kernels_split.txt)
        for (int i = tid; i < D; i += nth) if (zt[i] != zt[i]) flags[1] = 1;
        __syncthreads();
        const bool failed = flags[0] != 0, has_nan = flags[1] != 0;
        __syncthreads();
        if (failed) {
            for (int i = tid; i < D; i += nth) zt[i] = (T)0;
            status = BT_SOLVE_CHOL_FAILED;
            break;
        }
        if (!has_nan) break;
        status = BT_SOLVE_RETRIED;
    }
    __syncthreads();
    for (int i = tid; i < D; i += nth) {
        const int k = 6 * pd.perm[i / 6] + i % 6;
        a.dx[k] = (float)zt[i];
        if (PUB) dx_publish(a, k, (float)zt[i]);
    }
    if (tid == 0) a.status[0] = status;
    BT_PF(8);
    if (PROF && lane == 0 && (wave == 0 || wave == 2)) {        // measurement only: phase cycle counts of a critical and a helper wave
        long long *o = reinterpret_cast<long long *>(a.status + 4) + (wave ? 1 : 0) * 10;
        for (int i = 0; i < 10; ++i) o[i] = pf[i];
    }
#undef BT_PF
}

template <typename T, bool PROF>
__global__ __launch_bounds__(768) void k_solve_lds(PlanDev pd, StepArgs a) { solve_lds_body<T, PROF, false>(pd, a); }

// ------------------------------------------------------------------ k_solve_fused
// The LDS-resident factorisation with ONE phase and one barrier per level (levels of at most
// two columns: two-ended chains).  Updates are split by destination (ba_plan_solver.cpp, fz_*):
// "pending" = the destination column is factored in the very next level, "lazy" = later.
//   diagonal wave  one per column: lanes 0..35 apply the pending updates to the column's diagonal
//                  block (one element each) and publish it through LDS + a flag
//   row waves      64 panel rows of one column each (metadata stays scalar): every lane applies
//                  the pending update of its own row (or of y_j) in registers - all loads in
//                  flight before the first FMA - while the diagonal wave works, then picks up the
//                  block, factors it redundantly in registers and forward-substitutes its row
//   helper waves   the lazy updates of the level below (one row of a triple per thread) and its
//                  lazy y contributions
// Against k_solve_lds (two phases: factor | substitute) this removes a barrier, the store and
// reload of L_jj between the phases and the wait of the substitution for the slowest helper.
// The sweep is bounded by LDS throughput (~175 KB of 16-byte reads per level, with bank conflicts
// between the 288-byte blocks) about as much as by the 6x6 chain; see DESIGN.md section 6.
// [S | y] -> LDS in factor order by LDS-DMA (global_load_lds_dwordx4: no staging registers, every piece of the system in
// flight at once).  A 16-byte piece = third h of row r of block b, piece index 18 b + 3 r + h — which IS its place in the
// factor's LDS image (block b at 288 b bytes, rows of 48 bytes), so a wave instruction deposits 64 consecutive pieces at a
// wave-uniform base + lane * 16 as the instruction requires, each lane fetching from its own place in S.  Blocks that S
// holds transposed (its lower triangle, in the caller's pose order) and the diagonal blocks (upper triangle cleared,
// damping ba.py:67) are put right afterwards in LDS (sys_dma_fixup).  `bsrc`: the plan's blk_src, copied to LDS beforehand.
template <typename T>
__device__ __forceinline__ void sys_dma_issue(const PlanDev &pd, const StepArgs &a, T *Lw, const int *bsrc, int wave, int lane, int nw) {
    static_assert(sizeof(T) == 8, "double factor");
    const int total = pd.nnzb * 18;
    const unsigned D = (unsigned)pd.D;
    for (int k = wave; k * 64 < total; k += nw) {
        const int idx = k * 64 + lane;
        if (idx < total) {
            const int b = idx / 18, rem = idx - 18 * b, r = rem / 3, h = rem - 3 * r;
            const unsigned src = (unsigned)bsrc[b], rn = src >> 9, cn = (src >> 1) & 255u;
            const double *g = a.S + ((6u * rn + (unsigned)r) * D + 6u * cn + 2u * (unsigned)h);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                             (__attribute__((address_space(3))) void *)(Lw + (size_t)k * 128), 16, 0, 0);
        }
    }
}
// After the DMA: the blocks S holds transposed, one thread per (block of the list `trl`, row r < 5) — its up to five
// (r, c > r) / (c, r) swaps with all reads in flight before the writes —, and the damping of the diagonal (ba.py:67), one
// thread per diagonal element.  The upper triangles of the diagonal blocks stay as they came (S keeps its lower triangle
// only): nothing reads them — the column wave's lanes carry them along as dead values, the back substitution's preparation
// keeps L^-1 in registers.
template <typename T>
__device__ __forceinline__ void sys_dma_fixup(const PlanDev &pd, const StepArgs &a, T *Lw, const int *trl, int ntr, const int *col_ptr, double lm, bool zero_upper, int tid, int nth) {
    for (int it = tid; it < ntr * 5; it += nth) {
        const int li = it / 5, r = it - 5 * li;
        T *blk = Lw + trl[li] * 36;
        T lo[5], up[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) if (r + 1 + k < 6) { lo[k] = blk[6 * (r + 1 + k) + r]; up[k] = blk[6 * r + r + 1 + k]; }
#pragma unroll
        for (int k = 0; k < 5; ++k) if (r + 1 + k < 6) { blk[6 * (r + 1 + k) + r] = up[k]; blk[6 * r + r + 1 + k] = lo[k]; }
    }
    for (int it = tid; it < pd.D; it += nth) {
        T *dptr = Lw + col_ptr[it / 6] * 36 + 7 * (it % 6);
        const T x = *dptr;
        *dptr = x + ((T)a.ep + (T)lm * x);
    }
    if (zero_upper)
        for (int it = tid; it < pd.n * 15; it += nth) {
            const int jb = it / 15, e = it - 15 * jb, r = e >= 10 ? 5 : e >= 6 ? 4 : e >= 3 ? 3 : e >= 1 ? 2 : 1, c = e - r * (r - 1) / 2;
            Lw[col_ptr[jb] * 36 + 6 * c + r] = (T)0;
        }
}

// The whole load for the LDS-resident double-precision solvers: global memory in two round trips (the plan's tables — static,
// L2-resident — among them blk_src; then [S | y], which other chips' atomics have just accumulated and which comes from the
// memory side) instead of a register-staged load's chain of dependent ones (13.6k -> 9k cycles at 64 keyframes incl. the fix-up).
// Contains workgroup barriers; the caller's barrier after it covers the fix-up.  `col_ptr`: the LDS copy.
template <typename T>
__device__ __forceinline__ void lds_load_system_dma(const PlanDev &pd, const StepArgs &a, T *Lw, T *z, int *bsrc, int *trl, int *ntr, const int *col_ptr,
                                                    double lm, bool first, bool zero_upper, int tid, int nth) {
    const int wave = tid >> 6, lane = tid & 63, nw = nth >> 6, D = pd.D;
    const int yperm = tid < D ? pd.perm[tid / 6] : 0;
    if (first) {
        if (tid == 0) *ntr = 0;
        __syncthreads();
        for (int i = tid; i < pd.nnzb; i += nth) {
            const int src = pd.blk_src[i];
            bsrc[i] = src;
            if (src & 1) trl[atomicAdd(ntr, 1)] = i;          // the blocks S holds transposed (any order)
        }
    }
    __syncthreads();
    sys_dma_issue<T>(pd, a, Lw, bsrc, wave, lane, nw);
    if (tid < D) z[tid] = (T)a.y[6 * yperm + tid % 6];
    for (int i = tid + nth; i < D; i += nth) z[i] = (T)a.y[6 * pd.perm[i / 6] + i % 6];
    __syncthreads();                                      // (waits for the wave's DMA as well: vmcnt(0) in front of the barrier)
    sys_dma_fixup<T>(pd, a, Lw, trl, *ntr, col_ptr, lm, zero_upper, tid, nth);
}

constexpr int kFusedCols = 2;     // columns per level k_solve_fused and k_solve_pipe handle (two-ended chains); wider levels use k_solve_lds

// The back substitution's level table, behind zt: one 8-byte word per (level, column slot, lane group g), so that a lane finds
// everything the level asks of it at an address that depends on the level number alone — nothing to look up behind a record.
//   .x  col | #sub-blocks << 8 | kBsSync (barrier before this level: ba_plan_solver.cpp bs_sync) | kBsNoCol (the slot has no column)
//   .y  sub-block g of the column: its block index | its row's column << 16; kBsNone: the column has no sub-block g (block 0
//       and row 0 then: addresses that can be read, the values are thrown away)
// kBsPad empty levels come first (levels -kBsPad .. -1): the loop reads ahead without asking where it is.
// Built by every attempt (the sweep's tables lie where zt and this table go).  `row_idx`: the LDS copy.
constexpr int kBsSync = 1 << 16, kBsNoCol = 1 << 17, kBsNone = (int)0x80000000, kBsPad = 3;
__host__ __device__ inline size_t backsub_table_bytes(const PlanDev &pd) { return (size_t)(pd.nlev + kBsPad) * kFusedCols * 8 * sizeof(int2); }
__device__ __forceinline__ void backsub_table(const PlanDev &pd, int2 *tab, const int *row_idx, int tid, int nth) {
    for (int i = tid; i < (pd.nlev + kBsPad) * kFusedCols * 8; i += nth) {
        const int g = i & 7, ls = i >> 3, l = ls / kFusedCols - kBsPad, s = ls % kFusedCols;
        int2 w = make_int2(kBsNoCol, kBsNone);
        if (l >= 0) {
            const int4 mm = reinterpret_cast<const int4 *>(pd.fz_meta)[2 * (l * kMaxLevelCols + s)];      // col, diag pos, #sub-blocks
            const int sync = pd.bs_sync[l] ? kBsSync : 0;
            w.x |= sync;
            if (mm.x >= 0) {
                const int b = mm.y + 1 + g;
                w.x = mm.x | (mm.z << 8) | sync;
                if (g < mm.z) w.y = b | ((row_idx[b] & 255) << 16);
            }
        }
        tab[i] = w;
    }
}

// Back substitution of the LDS-resident factor (diagonal blocks hold L_jj with 1/l_cc on the
// diagonal, or the updated A_jj: RAW_DIAG): brings it into M form, then x_j = zt_j - sum_{i>j} M_ij x_i by levels, descending.
template <typename T, bool RAW_DIAG = false>
__device__ __forceinline__ void lds_back_substitute(const PlanDev &pd, T *Lw, T *z, T *zt, const int *row_idx,
                                                    const int *col_ptr, const int2 *tab, int tid, int nth, long long *tprof = nullptr) {
    const int nnzb = pd.nnzb, nlev = pd.nlev, wave = tid >> 6, lane = tid & 63;
    lds_backsub_prep<T, RAW_DIAG>(Lw, z, zt, row_idx, col_ptr, nnzb, tid, nth);
    __syncthreads();
    if (tprof) tprof[0] = tprof[1] = clock64();         // (one pass: L^-1 and the M form end together)
    // (c) x_j = zt_j - sum_{i>j} M_ij x_i, levels descending, ONE WAVE PER COLUMN SLOT and no barrier unless
    // the level reads an x_i another slot's wave wrote since the last barrier (kBsSync): on a two-ended chain
    // the two waves run down their chains independently.  lane = (component c) * 8 + g, one sub-block per lane
    // group g.  A lone wave stands still for a whole LDS round trip at every wait, so a level has ONE: its x.
    // The lane's word of the table is read two levels ahead, and with it (landed a level ago) the static operands
    // — zt_j, the six M entries — one level ahead; all of that is issued right behind the level's x reads, which
    // are waited for alone, and lands under the multiply-adds.  Lanes without a sub-block (and the lanes of c = 6, 7) read along at harmless
    // addresses and drop the product: no divergent branch in the level.  Columns of more than 8 sub-blocks look
    // their further rounds up in the loop.
    const int c = lane >> 3, g = lane & 7;
    if (__builtin_amdgcn_readfirstlane(wave) < kFusedCols) {
        const int2 *wtab = tab + (kBsPad * kFusedCols + wave) * 8 + g;
        struct Pre { int2 w; T m[6]; T ztj; };
        auto word = [&](int l) { return wtab[l * (kFusedCols * 8)]; };
        auto operands = [&](Pre &P) {                 // everything of the level of P.w that does not depend on the x computed so far
            P.ztj = zt[6 * (P.w.x & 255) + c];
            const T *mb = Lw + (P.w.y & 0x7fff) * 36 + c;             // Mt[r][c]
#pragma unroll
            for (int k = 0; k < 6; ++k) P.m[k] = mb[6 * k];
        };
        int2 wn;                                       // the word two levels ahead
        // one level: P holds its word and operands; N is filled for the level after it, behind this level's x in the queue
        auto level = [&](const Pre &P, Pre &N, int l2) {
            const int wx = __builtin_amdgcn_readfirstlane(P.w.x);
            if (wx & kBsSync) __syncthreads();
            T x[6];
            load_row6(zt + 6 * ((P.w.y >> 16) & 255), x);
            __builtin_amdgcn_sched_barrier(0);
            N.w = wn;
            wn = word(l2);
            operands(N);
            __builtin_amdgcn_sched_barrier(0);
            if (!(wx & kBsNoCol)) {
                const int j = wx & 255, cnt = (wx >> 8) & 255;
                T acc = P.m[0] * x[0] + P.m[1] * x[1] + P.m[2] * x[2] + P.m[3] * x[3] + P.m[4] * x[4] + P.m[5] * x[5];
                asm volatile("" : "+v"(acc));                        // (every lane forms it: no branch for the lanes that drop it)
                if (P.w.y < 0) acc = (T)0;
                if (cnt > 8 && c < 6)
                    for (int sb = g + 8, b = (P.w.y & 0x7fff) + 8; sb < cnt; sb += 8, b += 8) {       // wide columns: further sub-blocks of this lane group
                        load_row6(zt + 6 * (row_idx[b] & 255), x);
                        const T *mb = Lw + b * 36 + c;
                        acc += mb[0] * x[0] + mb[6] * x[1] + mb[12] * x[2] + mb[18] * x[3] + mb[24] * x[4] + mb[30] * x[5];
                    }
                acc = dpp_add8(acc);
                if (c < 6 && g == 0) zt[6 * j + c] = P.ztj - acc;
                wave_fence();
            }
        };
        Pre A = {}, B = {};                            // two register sets, levels alternate between them
        A.w = word(nlev - 1);
        wn = word(nlev - 2);
        operands(A);
        for (int l = nlev - 1; l >= 0; l -= 2) {       // (an odd count ends on an empty level of the padding)
            level(A, B, l - 2);
            level(B, A, l - 3);
        }
    } else {
        // (the other waves only keep the barriers company: the same for every slot of a level, so they follow slot 0)
        for (int l = nlev - 1; l >= 0; --l)
            if (__builtin_amdgcn_readfirstlane(tab[(kBsPad + l) * kFusedCols * 8].x) & kBsSync) __syncthreads();
    }
    __syncthreads();
}

// ---- what the sweeps of k_solve_fused and k_solve_pipe share (the probe macros stay with the kernels, between the calls)
// Where the first pending pair of the row wave's lane rw is found in pfirst: its own block, or the diagonal block for y_j and
// for the lanes without a row.  `ma`: the column's record word (col | #sub-blocks << 8 | ...), dpos: its diagonal block.
__device__ __forceinline__ int pfirst_index(int ma, int dpos, int rw) { return rw < ((ma >> 8) & 255) * 6 ? dpos + 1 + rw / 6 : dpos; }

// What a wave looks at in front of operands that other waves write.  look() issues the flag reads and passed() tests them, with
// the operand reads issued in between: the CU's LDS executes a wave's instructions in order and the producers drain their
// stores before they raise a flag, so operands read behind a flag that had the value are good — the first look that passes
// costs ONE round trip, not the flags' and then the operands'.  After a miss the operands are thrown away and both are read
// again.  The compiler keeps the order (and reads again in every round) because of the two barriers; checked in the ISA.
struct NoPoll {                                         // k_solve_fused: the workgroup barrier has ordered everything
    __device__ __forceinline__ void look() {}
    __device__ __forceinline__ bool passed() { return true; }
};
struct LevelPoll {                                      // k_solve_pipe, start of a level: colready[0] >= need0, colready[1] >= need1, hcnt >= needh
    int *colready, *hcnt;
    int need0, need1, needh, f0, f1, fh, lastfail;
    __device__ __forceinline__ void look() {
        f0 = __hip_atomic_load(&colready[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        f1 = __hip_atomic_load(&colready[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        fh = __hip_atomic_load(hcnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        asm volatile("" ::: "memory");
    }
    __device__ __forceinline__ bool passed() {
        asm volatile("" ::: "memory");
        if (f0 >= need0 && f1 >= need1 && fh >= needh) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            return true;
        }
        lastfail = fh < needh ? 1 : 0;                   // (PROF: what the wait was for: 1 = the helpers' batch, 0 = a column)
        __builtin_amdgcn_s_sleep(1);
        return false;
    }
};

// Row wave: the pending update of panel row rw of the column (record ma, diagonal block at dpos), or of y_j for rw = 6 cnt, in
// registers.  Returns where the row lives; `valid`: the lane has a row at all.  `pfo`: the lane's word of pfirst (pfirst_index).
template <typename T, typename Poll>
__device__ __forceinline__ T *row_wave_pending(T *Lw, T *z, const int *row_idx, unsigned pfo, const int *psecond, int ma, int dpos, int rw,
                                               bool &valid, T (&in)[6], Poll &poll) {
    const int j = ma & 255, cnt = (ma >> 8) & 255, ysrc = (ma >> 16) & 255;
    const bool isy = rw == cnt * 6;
    valid = rw <= cnt * 6;
    const int sb = rw / 6, r = rw - 6 * sb, bown = dpos + 1 + sb;
    T *p = isy ? z + 6 * j : Lw + (size_t)bown * 36 + 6 * r;
    // in[c] -= sum_e avec[e] M[c][e] with avec = row r of src1 and M = src2, or for the y row
    // avec = y of the source column and M = src1; every load is in flight before the first FMA
    const int s1 = pfo & 0x7fff, s2 = (pfo >> 15) & 0x7fff, no = valid ? (int)(pfo >> 30) : 0;
    T avec[6], m[36];
    const T *ap = isy ? z + 6 * ysrc : Lw + (size_t)s1 * 36 + 6 * r, *M = Lw + (size_t)(isy ? s1 : s2) * 36;
    auto look_and_load = [&]() {
        poll.look();
        load_row6(p, in);
        load_row6(ap, avec);
#pragma unroll
        for (int c = 0; c < 6; ++c) load_row6(M + 6 * c, reinterpret_cast<T (&)[6]>(m[6 * c]));
    };
    look_and_load();                                  // (the first look stands by itself: a loop's head waits for the wave's stores)
    while (!poll.passed()) look_and_load();
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        T acc = avec[0] * m[6 * c];
#pragma unroll
        for (int e = 1; e < 6; ++e) acc += avec[e] * m[6 * c + e];
        in[c] -= no > 0 ? acc : (T)0;
    }
    if (__builtin_amdgcn_ballot_w64(no > 1)) {       // where chains merge: a second pending pair
        const unsigned ps = (unsigned)psecond[isy ? dpos : bown];
        const int t1 = ps & 0x7fff, t2 = (ps >> 15) & 0x7fff;
        load_row6(isy ? z + 6 * ((row_idx[t1] >> 8) & 255) : Lw + (size_t)t1 * 36 + 6 * r, avec);
        const T *M = Lw + (size_t)(isy ? t1 : t2) * 36;
#pragma unroll
        for (int c = 0; c < 6; ++c) load_row6(M + 6 * c, reinterpret_cast<T (&)[6]>(m[6 * c]));
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            T acc = avec[0] * m[6 * c];
#pragma unroll
            for (int e = 1; e < 6; ++e) acc += avec[e] * m[6 * c + e];
            in[c] -= no > 1 ? acc : (T)0;
        }
    }
    return p;
}

// LDS of k_solve_fused and k_solve_pipe: Lw | z | work | row_idx | pfirst | col_ptr ..., where `work` holds the sweep's
// tables (published diagonal blocks, lazy triples) and is reused for zt afterwards.
// k_solve_fused leaves the per-level metadata in global memory (prefetched a level ahead).
__host__ __device__ inline size_t sweep_work_bytes(const PlanDev &pd) {
    const size_t b = 2 * 36 * sizeof(double) +          // published diagonal blocks of the level's two columns
                     (size_t)pd.fz_nlazy * 4 * sizeof(unsigned short) + 16;
    const size_t zt = (size_t)((pd.D + 1) & ~1) * sizeof(double) + backsub_table_bytes(pd);   // zt + the back substitution's level table
    return ((b > zt ? b : zt) + 15) / 16 * 16;
}
size_t solve_fused_lds_bytes(const PlanDev &pd, int) {
    return ((size_t)pd.nnzb * 36 + (size_t)pd.D) * sizeof(double) + sweep_work_bytes(pd) +
           (5 * (size_t)pd.nnzb + (size_t)pd.n + 1) * sizeof(int) + 64;       // row_idx, pfirst, psecond, col_ptr, bsrc, trl
}

template <bool PROF, bool PUB>
__device__ __forceinline__ void solve_fused_body(const PlanDev &pd, const StepArgs &a) {
    typedef double T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int flags[2];
    __shared__ int lready[kFusedCols];                 // level + 1 whose updated diagonal block is ready in scr
    __shared__ int ntr;
    __shared__ int4 mbuf[3][2];                        // packed level metadata, rolling: levels l, l+1, l+2
    const int tid = threadIdx.x, nth = blockDim.x, wave = tid >> 6, lane = tid & 63, nw = nth >> 6;
    const int n = pd.n, D = pd.D, nnzb = pd.nnzb, nlev = pd.nlev;
    T *Lw = reinterpret_cast<T *>(smem);
    // work region: per-column scratch (updated diagonal block, 36), lazy triples
    T *z = Lw + (size_t)nnzb * 36, *scr = z + D, *zt = scr;
    unsigned short *lazy = reinterpret_cast<unsigned short *>(scr + kFusedCols * 36);
    int *row_idx = reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(scr) + sweep_work_bytes(pd)), *pfirst = row_idx + nnzb,
        *psecond = pfirst + nnzb, *col_ptr = psecond + nnzb, *bsrc = col_ptr + n + 1, *trl = bsrc + nnzb;
    const int4 *pmeta = reinterpret_cast<const int4 *>(pd.fz_pmeta);     // [nlev][2]
    // per block: row | col << 8 | shared-y << 24 | pending-y << 25, and its first pending pair
    // src1 | src2 << 15 | count << 30, and the second pair (where chains merge) src1 | src2 << 15
    for (int i = tid; i < nnzb; i += nth) { row_idx[i] = pd.fz_rowinfo[i]; pfirst[i] = pd.fz_pfirst[i]; psecond[i] = pd.fz_psecond[i]; }
    for (int i = tid; i <= n; i += nth) col_ptr[i] = pd.col_ptr[i];
    long long phA = 0, phL = 0, tph = 0, tall = PROF ? clock64() : 0, tload = 0, tsweep = 0, sub[6] = {0, 0, 0, 0, 0, 0}, tsub = 0;
#define BT_SUB(i) do { if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long tq = clock64(); sub[i] += tq - tsub; tsub = tq; } } while (0)
    // (no barrier here: the load of S below does not read these tables; the barrier after it covers both)

    int status = BT_SOLVE_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const double lm = attempt == 0 ? 1e-4 : 1e-3;
        if (tid < 2) flags[tid] = 0;
        if (tid < kFusedCols) lready[tid] = 0;
        // the sweep's tables (their LDS is reused for zt by the back substitution, so a retry reloads them)
        for (int i = tid; i < pd.fz_nlazy; i += nth)          // one 8-byte word per triple: src1, src2, dst | shared << 15
            reinterpret_cast<ushort4 *>(lazy)[i] = make_ushort4((unsigned short)pd.fz_lazy[3 * i], (unsigned short)pd.fz_lazy[3 * i + 1],
                                                               (unsigned short)pd.fz_lazy[3 * i + 2], 0);
        if (tid < 4 && (tid >> 1) < nlev) mbuf[tid >> 1][tid & 1] = pmeta[tid];       // metadata of levels 0 and 1
        lds_load_system_dma<T>(pd, a, Lw, z, bsrc, trl, &ntr, col_ptr, lm, attempt == 0, true, tid, nth);
        __syncthreads();
        if (PROF) tload = clock64() - tall;

        // wave-uniform packed level metadata in SGPRs (ba_plan_solver.cpp: fz_pmeta): current, next and previous level
        int c0a, c0b, c0c, c0d, c1a, c1b, c1c, c1d, n0a = 0, n0b = 0, n0c = 0, n0d = 0, n1a = 0, n1b = 0, n1c = 0, n1d = 0;
        int p0a = 0, p0b = 0, p0c = 0, p1a = 0, p1b = 0, p1c = 0, pnc = 0;
        auto take_next = [&](int l) {
            const int4 m0 = mbuf[l % 3][0], m1 = mbuf[l % 3][1];
            n0a = __builtin_amdgcn_readfirstlane(m0.x); n0b = __builtin_amdgcn_readfirstlane(m0.y);
            n0c = __builtin_amdgcn_readfirstlane(m0.z); n0d = __builtin_amdgcn_readfirstlane(m0.w);
            n1a = __builtin_amdgcn_readfirstlane(m1.x); n1b = __builtin_amdgcn_readfirstlane(m1.y);
            n1c = __builtin_amdgcn_readfirstlane(m1.z); n1d = __builtin_amdgcn_readfirstlane(m1.w);
        };
        take_next(0);
        const bool feeder = tid >= nth - 2;           // the last two threads bring in level l + 2's metadata
        for (int l = 0; l < nlev; ++l) {
            c0a = n0a; c0b = n0b; c0c = n0c; c0d = n0d; c1a = n1a; c1b = n1b; c1c = n1c; c1d = n1d;
            if (PROF) tph = clock64();
            int4 mnext = make_int4(0, 0, 0, 0);
            if (feeder && l + 2 < nlev) mnext = pmeta[(size_t)(l + 2) * 2 + (tid - (nth - 2))];
            const int cnc = (c0b >> 24) & 3;
            const int nr0 = (c0b >> 16) & 255, nr1 = cnc > 1 ? (c1b >> 16) & 255 : 0;     // row waves of the two columns
            const int nA = cnc + nr0 + nr1;                                               // diagonal waves, then row waves
            for (int aw = wave; aw < nA; aw += nw) {
                __builtin_amdgcn_s_setprio(3);
                if (PROF) tsub = clock64();
                if (aw < cnc) {
                    // ---- diagonal wave of column q = aw: bring the diagonal block up to date with its pending
                    // updates (lanes 0..35, one element each) and publish it to the column's row waves
                    const int q = aw, dpos = (q ? c1b : c0b) & 0xffff, md = q ? c1d : c0d;
                    const int el = lane < 36 ? lane : lane - 36, dr = el / 6, dc = el - 6 * dr;
                    const int sd = md & 0x7fff, nd = (md >> 15) & 3;
                    T x[6], yv[6];
                    T v = Lw[(size_t)dpos * 36 + el];
                    load_row6(Lw + (size_t)sd * 36 + 6 * dr, x);
                    load_row6(Lw + (size_t)sd * 36 + 6 * dc, yv);
                    if (nd > 0) {
                        T acc = x[0] * yv[0];
#pragma unroll
                        for (int e = 1; e < 6; ++e) acc += x[e] * yv[e];
                        v -= acc;
                    }
                    if (nd > 1) {                         // where chains merge: a second pending pair (from the level's other column)
                        const T *src = Lw + (size_t)(psecond[dpos] & 0x7fff) * 36;
                        load_row6(src + 6 * dr, x);
                        load_row6(src + 6 * dc, yv);
                        T acc = x[0] * yv[0];
#pragma unroll
                        for (int e = 1; e < 6; ++e) acc += x[e] * yv[e];
                        v -= acc;
                    }
                    if (lane < 36) {
                        scr[q * 36 + lane] = v;
                        Lw[(size_t)dpos * 36 + lane] = v;          // in place as well: its next reader is the back substitution
                    }
                    // the row waves factor it themselves (their own pending update runs meanwhile)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    if (lane == 0) __hip_atomic_store(&lready[q], l + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    BT_SUB(0);
                    __builtin_amdgcn_s_setprio(0);
                } else {
                    // ---- row wave: one panel row (or y_j) per lane: its pending update, then, once the diagonal
                    // wave has published the updated block, its factorisation (every lane, in registers) and the
                    // forward substitution of the row
                    const int ra = aw - cnc, q = ra >= nr0 ? 1 : 0, part = ra - (q ? nr0 : 0);
                    const int ma = q ? c1a : c0a, dpos = (q ? c1b : c0b) & 0xffff;
                    bool valid;
                    T in[6];
                    NoPoll nopoll;
                    T *p = row_wave_pending(Lw, z, row_idx, (unsigned)pfirst[pfirst_index(ma, dpos, part * 64 + lane)], psecond, ma, dpos,
                                            part * 64 + lane, valid, in, nopoll);
                    BT_SUB(3);
                    while (__hip_atomic_load(&lready[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) <= l) __builtin_amdgcn_s_sleep(1);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    T L[21];
                    {
                        const T *dblk = scr + q * 36;
#pragma unroll
                        for (int rr = 0; rr < 6; ++rr) {
                            T row[6];
                            load_row6(dblk + 6 * rr, row);
#pragma unroll
                            for (int c = 0; c <= rr; ++c) L[BT_LT(rr, c)] = row[c];
                        }
                    }
                    const bool ok = chol6_packed<T>(L);
                    if (!ok && part == 0 && lane == 0) flags[0] = 1;
                    BT_SUB(4);
                    if (valid) {
                        T out[6];
#pragma unroll
                        for (int c = 0; c < 6; ++c) {
                            T t = in[c];
#pragma unroll
                            for (int k = 0; k < c; ++k) t -= out[k] * L[BT_LT(c, k)];
                            out[c] = t * L[BT_LT(c, c)];
                        }
                        store_row6(p, out);
                    }
                    BT_SUB(5);
                    __builtin_amdgcn_s_setprio(0);
                }
            }
            if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long tn = clock64(); phA += tn - tph; tph = tn; }
            // ---- lazy updates of the level below: helper waves (all waves once there are more column waves than waves)
            if (l > 0) {
                int h, hs;
                if (nA < nw) { h = tid - 64 * nA; hs = nth - 64 * nA; }
                else { hs = nth; h = (tid + nth - (64 * nA) % nth) % nth; }
                if (h >= 0) {
                    const int rows0 = ((p0c >> 16) & 0xffff) * 6, rows1 = rows0 + (pnc > 1 ? ((p1c >> 16) & 0xffff) * 6 : 0);
                    for (int item = h; item < rows1; item += hs) {
                        const bool sec = item >= rows0;
                        const int idx = item - (sec ? rows0 : 0), t = idx / 6;
                        const ushort4 tr = reinterpret_cast<const ushort4 *>(lazy)[((sec ? p1c : p0c) & 0xffff) + t];
                        apply_update_row3<T>(Lw, tr.x, tr.y, tr.z, idx - 6 * t);
                    }
                    // lazy y contributions of the level below, on the threads after those with update rows
                    {
                        const int ys0 = ((p0a >> 8) & 255) * 6, ys1 = ys0 + (pnc > 1 ? ((p1a >> 8) & 255) * 6 : 0);
                        const int shift = ((rows1 + 63) >> 6) << 6;
                        int first = h - shift;                       // (no division in the usual one-round case)
                        if (shift > hs) first = (h - shift % hs + hs) % hs; else if (first < 0) first += hs;
                        for (int item = first; item < ys1; item += hs) {
                            const bool sec = item >= ys0;
                            const int qq = item - (sec ? ys0 : 0);
                            const int pj = (sec ? p1a : p0a) & 255, dposp = (sec ? p1b : p0b) & 0xffff, sb = qq / 6, r = qq - 6 * sb;
                            const int rcv = row_idx[dposp + 1 + sb];
                            if (rcv & (1 << 25)) continue;            // pending: the destination column's y thread takes it
                            T lr[6], zr[6];
                            load_row6(Lw + (size_t)(dposp + 1 + sb) * 36 + 6 * r, lr);
                            load_row6(z + 6 * pj, zr);
                            T acc = lr[0] * zr[0];
#pragma unroll
                            for (int k = 1; k < 6; ++k) acc += lr[k] * zr[k];
                            lds_sub(z + 6 * (rcv & 255) + r, acc, (rcv & (1 << 24)) != 0);
                        }
                    }
                }
            }
            if (feeder && l + 2 < nlev) mbuf[(l + 2) % 3][tid - (nth - 2)] = mnext;
            if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); phL += clock64() - tph; }
            p0a = c0a; p0b = c0b; p0c = c0c; p1a = c1a; p1b = c1b; p1c = c1c; pnc = cnc;
            if (l + 1 < nlev) take_next(l + 1);
            __syncthreads();
        }
        if (PROF) tsweep = clock64() - tall;

        int2 *btab = reinterpret_cast<int2 *>(zt + ((D + 1) & ~1));          // the level table behind zt
        backsub_table(pd, btab, row_idx, tid, nth);
        long long tbs[2] = {0, 0};
        lds_back_substitute<T, true>(pd, Lw, z, zt, row_idx, col_ptr, btab, tid, nth, PROF ? tbs : nullptr);
        if (PROF) { sub[0] = tbs[0] - tall; sub[1] = tbs[1] - tall; sub[2] = clock64() - tall; }
        for (int i = tid; i < D; i += nth) if (zt[i] != zt[i]) flags[1] = 1;
        __syncthreads();
        const bool failed = flags[0] != 0, has_nan = flags[1] != 0;
        __syncthreads();
        if (failed) {
            for (int i = tid; i < D; i += nth) zt[i] = (T)0;
            status = BT_SOLVE_CHOL_FAILED;
            break;
        }
        if (!has_nan) break;
        status = BT_SOLVE_RETRIED;
    }
    __syncthreads();
    for (int i = tid; i < D; i += nth) {
        const int k = 6 * pd.perm[i / 6] + i % 6;
        a.dx[k] = (float)zt[i];
        if (PUB) dx_publish(a, k, (float)zt[i]);
    }
    if (tid == 0) a.status[0] = status;
    if (PROF && lane == 0) {        // measurement only: per-wave busy cycles (columns, lazy work) and the stage boundaries
        long long *o = reinterpret_cast<long long *>(a.status + 4) + 40 + wave * 2;
        o[0] = phA; o[1] = phL;
        if (wave == 0 || wave == 2) {
            long long *g = reinterpret_cast<long long *>(a.status + 4) + (wave ? 10 : 0);
            g[0] = tload; g[1] = tsweep; g[2] = clock64() - tall;
            for (int i = 0; i < 6; ++i) g[3 + i] = sub[i];       // wave 0: end of the back-substitution preparation (twice: it was two phases) and of the back substitution; wave 2: row-wave stages
        }
    }
#undef BT_SUB
}

template <bool PROF>
__global__ __launch_bounds__(768) void k_solve_fused(PlanDev pd, StepArgs a) { solve_fused_body<PROF, false>(pd, a); }

// ------------------------------------------------------------------ k_solve_pipe
// k_solve_fused without the per-level workgroup barrier.  Waves have fixed roles and walk the levels at
// their own pace, ordered by flags in LDS only where data flows:
//   wave q (q = 0, 1)      diagonal wave of the level's column q      -> lready[q]   = level + 1
//   wave 2 + q             row wave of column q (panel rows and y_j)   -> colready[q] = level + 1
//   waves 4 ..             helpers: batch b = the lazy updates whose sources are the columns of level b;
//                          every helper wave adds 1 to hcnt when it has finished its share of a batch
// What a step waits for (tests/plan_emulator.py checks that these waits order every conflicting access):
//   column waves, level l   colready[s] >= l for the columns s of level l - 1 that hold pending sources of this
//                           column (on a chain: its own predecessor only, so the two chains do not wait for
//                           each other) and hcnt >= nh (l - 1): batches 0 .. l - 2 are complete, i.e. every
//                           lazy update into this level's blocks has landed
//   row wave                additionally lready[q] >= l + 1 before it factors
//   helpers, batch b        colready[*] >= b + 1 for the columns of level b (its sources) and
//                           hcnt >= nh b (the whole group has finished the batches before: two batches may
//                           read-modify-write the same destination row from different waves)
// A chain's row wave therefore never waits for anything but its diagonal wave in steady state; the barrier
// (~240 cycles by itself) and the wait for the slowest wave of every level are gone.  What it does pay for is every LDS
// round trip it stands still for (a lone wave, and eight helper waves keep the LDS busy), so a level of the row wave has two:
// its flags with the operands of its pending update behind them, and lready with the published block behind it (LevelPoll);
// the lane's pfirst word and the next level's record are read a level ahead, under the factorisation
// (profiles/r24_solver_round_trips.txt).  Requires columns of at
// most 64 panel rows and levels of at most two columns (plan flag fzp_ok); other systems use k_solve_fused.
size_t solve_pipe_lds_bytes(const PlanDev &pd) {
    return ((size_t)pd.nnzb * 36 + (size_t)pd.D) * sizeof(double) + sweep_work_bytes(pd) +
           (5 * (size_t)pd.nnzb + (size_t)pd.n + 1 + (size_t)pd.nlev * 8) * sizeof(int) + 64;      // row_idx, pfirst, psecond, col_ptr, level records, bsrc, trl
}

__device__ __forceinline__ void wait_ge(int *flag, int target) {
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
}

template <bool PROF, bool PUB>
__device__ __forceinline__ void solve_pipe_body(const PlanDev &pd, const StepArgs &a) {
    typedef double T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int flags[2];
    __shared__ int lready[2], colready[2], hcnt, ntr;
    const int tid = threadIdx.x, nth = blockDim.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nw = nth >> 6;
    const int n = pd.n, D = pd.D, nnzb = pd.nnzb, nlev = pd.nlev;
    T *Lw = reinterpret_cast<T *>(smem);
    T *z = Lw + (size_t)nnzb * 36, *scr = z + D, *zt = scr;
    unsigned short *lazy = reinterpret_cast<unsigned short *>(scr + 2 * 36);
    int *row_idx = reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(scr) + sweep_work_bytes(pd)), *pfirst = row_idx + nnzb,
        *psecond = pfirst + nnzb, *col_ptr = psecond + nnzb, *lrec = col_ptr + n + 1, *bsrc = lrec + nlev * 8, *trl = bsrc + nnzb;
    for (int i = tid; i < nnzb; i += nth) { row_idx[i] = pd.fz_rowinfo[i]; pfirst[i] = pd.fz_pfirst[i]; psecond[i] = pd.fz_psecond[i]; }
    for (int i = tid; i <= n; i += nth) col_ptr[i] = pd.col_ptr[i];
    for (int i = tid; i < nlev * 8; i += nth) lrec[i] = pd.fz_pmeta[i];
    long long tall = PROF ? clock64() : 0, tload = 0, tsweep = 0, twait = 0, twork = 0, tq = 0, sub[3] = {0, 0, 0}, wsplit[2] = {0, 0};
#define BT_TW(acc) do { if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const long long tn = clock64(); acc += tn - tq; tq = tn; } } while (0)

    int status = BT_SOLVE_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const double lm = attempt == 0 ? 1e-4 : 1e-3;
        if (tid < 2) { flags[tid] = 0; lready[tid] = 0; colready[tid] = 0; }
        if (tid == 2) hcnt = 0;
        int nlazy = pd.fz_nlazy;
        // (inside k_solve_update the copy loop's trip count, hoisted out of the attempt loop, was the one value the register
        //  allocator spilled: 8 bytes of scratch per lane that k_solve_pipe alone does not have, 0 with the value opaque here and
        //  formed per attempt — compiler figures in profiles/r22_solve_update.txt.  k_solve_pipe itself compiles as before.)
        asm volatile("" : "+s"(nlazy));
        for (int i = tid; i < nlazy; i += nth)                // one 8-byte word per triple: src1, src2, dst | shared << 15
            reinterpret_cast<ushort4 *>(lazy)[i] = make_ushort4((unsigned short)pd.fz_lazy[3 * i], (unsigned short)pd.fz_lazy[3 * i + 1],
                                                               (unsigned short)pd.fz_lazy[3 * i + 2], 0);
        lds_load_system_dma<T>(pd, a, Lw, z, bsrc, trl, &ntr, col_ptr, lm, attempt == 0, true, tid, nth);
        __syncthreads();
        if (PROF) { tload = clock64() - tall; tq = clock64(); }

        const int nh = nw - 4;                                   // helper waves
        if (wave < 4) {
            // ================= column waves: q = wave & 1, diagonal wave (wave < 2) or row wave
            const int q = wave & 1;
            const bool is_row = wave >= 2;
            const int4 *lrec4 = reinterpret_cast<const int4 *>(lrec);
            int4 vrec = lrec4[q];                                // this wave's record and slot 0's (it carries the number of columns)
            int vnc = lrec[1];
            int npc = 0;                                         // columns of the level below
            // row wave: the lane's word of pfirst, read a level ahead (its address needs the level's record alone, which is
            // here a level ahead too) and carried in a register: the operand reads of a level follow its flags directly
            unsigned pfn = is_row ? (unsigned)pfirst[pfirst_index(vrec.x, vrec.y & 0xffff, lane)] : 0u;
            for (int l = 0; l < nlev; ++l) {
                const int ma = __builtin_amdgcn_readfirstlane(vrec.x), mb = __builtin_amdgcn_readfirstlane(vrec.y),
                          md = __builtin_amdgcn_readfirstlane(vrec.w), ncl = (__builtin_amdgcn_readfirstlane(vnc) >> 24) & 3;
                // next level's record, in flight during this one (the row wave asks for it once its operands are in registers:
                // during their reads every register counts)
                auto next_record = [&]() { if (l + 1 < nlev) { vrec = lrec4[2 * (l + 1) + q]; vnc = lrec[8 * (l + 1) + 1]; } };
                if (!is_row) next_record();
                if (q < ncl) {
                    // What the level waits for: only the columns of the level below that hold pending sources of this column
                    // (the record's dependency bits: on a chain its own predecessor, which this very row wave wrote) and the
                    // helpers' batches; the three flags and the operands behind them in one LDS round trip (LevelPoll)
                    // (the diagonal wave also waits for the row wave that last read its scratch slot)
                    const int dep = l > 0 ? ((md >> 20) & 3) | ((!is_row && q < npc) ? 1 << q : 0) : 0;
                    LevelPoll poll = {colready, &hcnt, (dep & 1) ? l : 0, (dep & 2) ? l : 0, l > 0 ? nh * (l - 1) : 0, 0, 0, 0, -1};
                    const long long tw0 = PROF ? clock64() : 0;
                    const int dpos = mb & 0xffff;
                    if (!is_row) {
                        // ---- diagonal wave: bring the diagonal block up to date with its pending updates (lanes 0..35,
                        // one element each) and publish it to the row wave
                        // (same text in k_solve_fused but for the poll: as one function it changed both kernels' instruction streams (resources equal); not measured on the GPU, so it stays twice -- profiles/r15_kernels_split.txt)
                        const int el = lane < 36 ? lane : lane - 36, dr = el / 6, dc = el - 6 * dr;
                        const int sd = md & 0x7fff, nd = (md >> 15) & 3;
                        T x[6], yv[6];
                        T v;
                        // (the flags alone, then the operands: this wave is ahead of its row wave and misses nearly every first
                        //  look; with the seven operand reads in every round the C3 solve measured 0.8 us slower)
                        do poll.look(); while (!poll.passed());
                        v = Lw[(size_t)dpos * 36 + el];
                        load_row6(Lw + (size_t)sd * 36 + 6 * dr, x);
                        load_row6(Lw + (size_t)sd * 36 + 6 * dc, yv);
                        if (PROF && poll.lastfail >= 0) wsplit[poll.lastfail] += clock64() - tw0;
                        BT_TW(twait);
                        if (nd > 0) {
                            T acc = x[0] * yv[0];
#pragma unroll
                            for (int e = 1; e < 6; ++e) acc += x[e] * yv[e];
                            v -= acc;
                        }
                        if (nd > 1) {                         // where chains merge: a second pending pair (from the level's other column)
                            const T *src = Lw + (size_t)(psecond[dpos] & 0x7fff) * 36;
                            load_row6(src + 6 * dr, x);
                            load_row6(src + 6 * dc, yv);
                            T acc = x[0] * yv[0];
#pragma unroll
                            for (int e = 1; e < 6; ++e) acc += x[e] * yv[e];
                            v -= acc;
                        }
                        if (lane < 36) {
                            scr[q * 36 + lane] = v;
                            Lw[(size_t)dpos * 36 + lane] = v;          // in place as well: its next reader is the back substitution
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        if (lane == 0) __hip_atomic_store(&lready[q], l + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        BT_TW(twork);
                    } else {
                        // ---- row wave: one panel row (or y_j) per lane: its pending update, then, once the diagonal wave
                        // has published the updated block, its factorisation (every lane, in registers) and the forward
                        // substitution of the row
                        bool valid;
                        T in[6];
                        T *p = row_wave_pending(Lw, z, row_idx, pfn, psecond, ma, dpos, lane, valid, in, poll);
                        if (PROF && poll.lastfail >= 0) wsplit[poll.lastfail] += clock64() - tw0;
                        BT_TW(sub[0]);
                        // (the factorisation and the substitution below: same text in k_solve_fused but for the poll: as one function it changed both kernels' instruction streams (resources equal); not measured on the GPU, so it stays twice -- profiles/r15_kernels_split.txt)
                        T L[21];
                        int lrf;
                        auto look_and_load = [&]() {            // lready[q], and the published block behind it in the same round trip
                            lrf = __hip_atomic_load(&lready[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            asm volatile("" ::: "memory");
                            const T *dblk = scr + q * 36;
#pragma unroll
                            for (int rr = 0; rr < 6; ++rr) {
                                T row[6];
                                load_row6(dblk + 6 * rr, row);
#pragma unroll
                                for (int c = 0; c <= rr; ++c) L[BT_LT(rr, c)] = row[c];
                            }
                            next_record();                      // (static, behind the block in the same round trip)
                            asm volatile("" ::: "memory");
                        };
                        look_and_load();
                        while (lrf <= l) { __builtin_amdgcn_s_sleep(1); look_and_load(); }       // (waits for lready[q] >= l + 1)
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                        if (l + 1 < nlev) pfn = (unsigned)pfirst[pfirst_index(vrec.x, vrec.y & 0xffff, lane)];      // (lands under the factorisation)
                        BT_TW(sub[1]);
                        const bool ok = chol6_packed<T>(L);
                        // (substitution computed by every lane, only the store is predicated: one basic block, so the
                        //  compiler can slot its FMAs into the latency gaps of the factorisation)
                        T out[6];
#pragma unroll
                        for (int c = 0; c < 6; ++c) {
                            T t = in[c];
#pragma unroll
                            for (int k = 0; k < c; ++k) t -= out[k] * L[BT_LT(c, k)];
                            out[c] = t * L[BT_LT(c, c)];
                        }
                        if (valid) store_row6(p, out);
                        if (!ok && lane == 0) flags[0] = 1;
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        if (lane == 0) __hip_atomic_store(&colready[q], l + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        BT_TW(sub[2]);
                    }
                } else if (is_row && l + 1 < nlev) {
                    next_record();
                    pfn = (unsigned)pfirst[pfirst_index(vrec.x, vrec.y & 0xffff, lane)];
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pfn));       // (here, not at the top of every level)
                }
                npc = ncl;
            }
        } else {
            // ================= helper waves: batch b = lazy updates and lazy y contributions of the columns of level b
            const int h = tid - 256, hs = nth - 256;
            for (int b = 0; b + 1 < nlev; ++b) {
                const int p0a = __builtin_amdgcn_readfirstlane(lrec[8 * b]), p0b = __builtin_amdgcn_readfirstlane(lrec[8 * b + 1]),
                          p0c = __builtin_amdgcn_readfirstlane(lrec[8 * b + 2]), p1a = __builtin_amdgcn_readfirstlane(lrec[8 * b + 4]),
                          p1b = __builtin_amdgcn_readfirstlane(lrec[8 * b + 5]), p1c = __builtin_amdgcn_readfirstlane(lrec[8 * b + 6]);
                const int pnc = (p0b >> 24) & 3;
                {
                    const int need1 = pnc > 1 ? b + 1 : 0;
                    for (;;) {
                        const int f0 = __hip_atomic_load(&colready[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        const int f1 = __hip_atomic_load(&colready[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        const int fh = __hip_atomic_load(&hcnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (f0 >= b + 1 && f1 >= need1 && fh >= nh * b) break;
                        __builtin_amdgcn_s_sleep(1);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                BT_TW(twait);
                // (same text in k_solve_fused: as one function it changed both kernels' instruction streams (resources equal); not measured on the GPU, so it stays twice -- profiles/r15_kernels_split.txt)
                const int rows0 = ((p0c >> 16) & 0xffff) * 6, rows1 = rows0 + (pnc > 1 ? ((p1c >> 16) & 0xffff) * 6 : 0);
                for (int item = h; item < rows1; item += hs) {
                    const bool sec = item >= rows0;
                    const int idx = item - (sec ? rows0 : 0), t = idx / 6;
                    const ushort4 tr = reinterpret_cast<const ushort4 *>(lazy)[((sec ? p1c : p0c) & 0xffff) + t];
                    apply_update_row3<T>(Lw, tr.x, tr.y, tr.z, idx - 6 * t);
                }
                {
                    const int ys0 = ((p0a >> 8) & 255) * 6, ys1 = ys0 + (pnc > 1 ? ((p1a >> 8) & 255) * 6 : 0);
                    const int shift = ((rows1 + 63) >> 6) << 6;
                    int first = h - shift;                       // (no division in the usual one-round case)
                    if (shift > hs) first = (h - shift % hs + hs) % hs; else if (first < 0) first += hs;
                    for (int item = first; item < ys1; item += hs) {
                        const bool sec = item >= ys0;
                        const int qq = item - (sec ? ys0 : 0);
                        const int pj = (sec ? p1a : p0a) & 255, dposp = (sec ? p1b : p0b) & 0xffff, sb = qq / 6, r = qq - 6 * sb;
                        const int rcv = row_idx[dposp + 1 + sb];
                        if (rcv & (1 << 25)) continue;            // pending: the destination column's y thread takes it
                        T lr[6], zr[6];
                        load_row6(Lw + (size_t)(dposp + 1 + sb) * 36 + 6 * r, lr);
                        load_row6(z + 6 * pj, zr);
                        T acc = lr[0] * zr[0];
#pragma unroll
                        for (int k = 1; k < 6; ++k) acc += lr[k] * zr[k];
                        lds_sub(z + 6 * (rcv & 255) + r, acc, (rcv & (1 << 24)) != 0);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if (lane == 0) __hip_atomic_fetch_add(&hcnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                BT_TW(twork);
            }
        }
        __syncthreads();
        if (PROF) tsweep = clock64() - tall;

        // (same text in k_solve_fused: as one function it changed both kernels' instruction streams (and k_solve_fused<false>'s registers, 167 -> 168); not measured on the GPU, so it stays twice -- profiles/r15_kernels_split.txt)
        int2 *btab = reinterpret_cast<int2 *>(zt + ((D + 1) & ~1));          // the level table behind zt
        backsub_table(pd, btab, row_idx, tid, nth);
        lds_back_substitute<T, true>(pd, Lw, z, zt, row_idx, col_ptr, btab, tid, nth, nullptr);
        for (int i = tid; i < D; i += nth) if (zt[i] != zt[i]) flags[1] = 1;
        __syncthreads();
        const bool failed = flags[0] != 0, has_nan = flags[1] != 0;
        __syncthreads();
        if (failed) {
            for (int i = tid; i < D; i += nth) zt[i] = (T)0;
            status = BT_SOLVE_CHOL_FAILED;
            break;
        }
        if (!has_nan) break;
        status = BT_SOLVE_RETRIED;
    }
    __syncthreads();
    for (int i = tid; i < D; i += nth) {
        const int k = 6 * pd.perm[i / 6] + i % 6;
        a.dx[k] = (float)zt[i];
        if (PUB) dx_publish(a, k, (float)zt[i]);
    }
    if (tid == 0) a.status[0] = status;
    if (PROF && lane == 0) {        // measurement only: per-wave (waiting, working) cycles of the sweep
        long long *o = reinterpret_cast<long long *>(a.status + 4) + 40 + wave * 2;
        o[0] = twait; o[1] = twork + sub[0] + sub[2];
        if (wave == 0 || wave == 2) {
            long long *g = reinterpret_cast<long long *>(a.status + 4) + (wave ? 10 : 0);
            g[0] = tload; g[1] = tsweep; g[2] = clock64() - tall;
            g[3] = sub[0]; g[4] = sub[1]; g[5] = sub[2]; g[6] = twait; g[7] = wsplit[0]; g[8] = wsplit[1];
        }
    }
#undef BT_TW
}

template <bool PROF>
__global__ __launch_bounds__(768) void k_solve_pipe(PlanDev pd, StepArgs a) { solve_pipe_body<PROF, false>(pd, a); }

// ------------------------------------------------------------------ refinement of float32-factor solves
// Systems whose factor does not fit LDS as double are factored in float32 (k_solve_lds<float>, k_solve_global): dX is then
// 5e-5 .. 1e-4 off the exact solution of [S | y] — outside the parity contract.  Iterative refinement, only for those systems:
// r = y - A dX0 in double from the S still in global memory (A = S + (ep + lm S) I, ba.py:67, with the lm the first solve
// ended on), the same solver once more on r, dX = dX0 + delta — TWICE (kRefineSteps): a step shrinks the error by
// cond(A) * 6e-8 * a small constant, and the 100-300-pose graphs that land here reach cond(A) = 3e5 with ep = 10, where one
// step left dX 9.4e-6 and the pose update 1.1e-5 from the float64 solve (tests/gpu_seed_probe.py, seed 32862) — outside the
// 1e-5 of the contract; two leave it at the float32 rounding of dX.  y holds the current residual throughout
// (r_{p+1} = r_p - A delta_p), dx0 the sum so far.  A failed factorisation gives 0 + 0 + 0 (ba.py:9-13).
// The second step is skipped where the first already converged: a step's correction is the error before it, the error after it
// that correction times the same contraction rho = |delta_1| / |dX0| — so |delta_1| <= 1.5e-4 |dX0| means the sum is within
// 2.3e-8 of the float64 solve, the float32 rounding of dX.  The residual kernel of the second step raises kRefineDone, the solve
// behind it returns at once and k_refine_add takes the sum as it is (a well-conditioned band pays two solves, not three).
constexpr int kRefineSteps = 2;
__global__ __launch_bounds__(256) void k_refine_residual(PlanDev pd, StepArgs a, int accumulate) {
    const int D = pd.D, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + w;
    if (i >= D) return;
    const double lm = a.status[0] == BT_SOLVE_RETRIED ? 1e-3 : 1e-4;
    double acc = 0.0;
    for (int j = lane; j < D; j += 64) {
        double s = i >= j ? a.S[(size_t)i * D + j] : a.S[(size_t)j * D + i];            // S holds the lower triangle
        if (i == j) s = s + ((double)a.ep + lm * s);
        acc += s * (double)a.dx[j];
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) a.y[i] = a.y[i] - acc;
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        double nd = 0.0, nx = 0.0;
        for (int k = threadIdx.x; k < D; k += 64) {
            const float d = a.dx[k], x = accumulate ? a.dx0[k] : 0.0f;
            nd += (double)d * d; nx += (double)x * x;
            a.dx0[k] = accumulate ? x + d : d;
        }
        for (int o = 32; o > 0; o >>= 1) { nd += __shfl_xor(nd, o); nx += __shfl_xor(nx, o); }
        if (threadIdx.x == 0) a.status[kRefineDone] = (accumulate && nd <= 2.25e-8 * nx) ? 1 : 0;      // (NaN: not done)
    }
}

// (one workgroup: it reads the flag, and clears it for the next step's first solve when everybody has)
__global__ __launch_bounds__(1024) void k_refine_add(PlanDev pd, StepArgs a) {
    const bool done = a.status[kRefineDone] != 0;
    for (int k = threadIdx.x; k < pd.D; k += blockDim.x) a.dx[k] = done ? a.dx0[k] : a.dx0[k] + a.dx[k];
    __syncthreads();
    if (threadIdx.x == 0) a.status[kRefineDone] = 0;
}

// ------------------------------------------------------------------ the solver of a route (fn == nullptr: the dense one)
Pick pick_solver(const PlanDev &pd, bool prof) {
    switch (pd.route.solver) {
    case Route::kSolvePipe:
        return prof ? pick_of<&k_solve_pipe<true>>(kSolveThreads, solve_pipe_lds_bytes(pd)) : pick_of<&k_solve_pipe<false>>(kSolveThreads, solve_pipe_lds_bytes(pd));
    case Route::kSolveFused: {
        const size_t lds = solve_fused_lds_bytes(pd, kSolveThreads);
        return prof ? pick_of<&k_solve_fused<true>>(kSolveThreads, lds) : pick_of<&k_solve_fused<false>>(kSolveThreads, lds);
    }
    case Route::kSolveLds: {
        const size_t lds = solve_lds_bytes(pd, sizeof(double));
        return prof ? pick_of<&k_solve_lds<double, true>>(kSolveThreads, lds) : pick_of<&k_solve_lds<double, false>>(kSolveThreads, lds);
    }
    case Route::kSolveLds32: {
        const size_t lds = solve_lds_bytes(pd, sizeof(float));
        return prof ? pick_of<&k_solve_lds<float, true>>(kSolveThreads, lds) : pick_of<&k_solve_lds<float, false>>(kSolveThreads, lds);
    }
    case Route::kSolveGlobal: return pick_of<&k_solve_global>(1024, 0);
    default: return Pick{};
    }
}

// the route's block-sparse solver; ev: the (start, stop) event pair of kernel 3 or nullptr (it times the first pass)
int launch_solve(const PlanDev &pd, const StepArgs &a, hipStream_t st, const hipEvent_t *ev) {
    const Route &r = pd.route;
    const Pick p = pick_solver(pd, (a.dbg & 16) != 0);
    const bool f32 = r.solver == Route::kSolveLds32 || r.solver == Route::kSolveGlobal;
    const int passes = f32 ? 1 + kRefineSteps : 1;             // float32 factor: iterative refinement
    for (int pass = 0; pass < passes; ++pass) {
        if (pass >= 1) hipLaunchKernelGGL(k_refine_residual, dim3((pd.D + 3) / 4), dim3(256), 0, st, pd, a, pass > 1 ? 1 : 0);
        launch_pick(p, 1, st, pass == 0 ? ev : nullptr, pd, a);
        if (pass >= 1 && pass == passes - 1) hipLaunchKernelGGL(k_refine_add, dim3(1), dim3(1024), 0, st, pd, a);
    }
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

}  // namespace bt

// The fused solve + update launch runs the solver bodies above in its first workgroup: device functions do not link across
// objects, so its header is part of this translation unit (and of no other).
#include "ba_solve_update.hpp"
