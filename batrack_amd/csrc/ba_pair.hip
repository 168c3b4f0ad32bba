// ba_pair.hip — k_pair_finalize: B and v of the reduced camera system (ba.py:279-290) from the per-pair sums the Jacobian
// kernels leave (gfx950, wave64).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "ba_kernels.hpp"

namespace bt {

// ------------------------------------------------------------------ k_pair_finalize
// One wave per camera pair, in double.  sym index of (p<=q) in the 21-vector:
__device__ __forceinline__ int sym21(int p, int q) {
    if (p > q) { const int t = p; p = q; q = t; }
    return p * 6 - p * (p - 1) / 2 + (q - p);
}

// Blocks behind the pair blocks (plans with sp_ok, Jacobian kernel k_etile): per group of consecutive same-camera tiles, one
// block per 16x16 tile of the Schur product E Q E^T (its 256 threads one element each, summed over the group's tiles in
// tile order: independent loads, eight in flight) and one for E Q w'; subtracted from [S | y] — a few atomics per element
// and step instead of one per element and TILE.
__global__ __launch_bounds__(256) void k_pair_finalize(PlanDev pd, StepArgs a, int pair_blocks) {
    if ((int)blockIdx.x >= pair_blocks) {
        const int R16 = pd.max_rows16, nt = R16 >> 4, ntl = nt * (nt + 1) / 2;
        const int g = ((int)blockIdx.x - pair_blocks) / (ntl + 1), b = ((int)blockIdx.x - pair_blocks) - g * (ntl + 1);
        const size_t per_tile = sp_tile_doubles(pd.max_rows16, pd.max_tile_pairs);
        const int t0 = pd.sg_ptr[g], t1 = pd.sg_ptr[g + 1];
        const int *cams = pd.tile_cams + pd.tile_cam0[t0];           // the cameras of every tile of the group
        const int Rw = 6 * pd.tile_ncam[t0];
        auto grow = [&](int r) { return 6 * cams[r / 6] + r % 6; };
        auto group_sum = [&](const double *src) {
            double sum = 0.0;
            for (int t = t0; t < t1; t += 8) {
                double v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = t + k < t1 ? src[(size_t)(t + k) * per_tile] : 0.0;
#pragma unroll
                for (int k = 0; k < 8; ++k) sum += v[k];
            }
            return sum;
        };
        if (b < ntl) {
            int ti = 0, base = 0;
            while (base + ti + 1 <= b) { base += ti + 1; ++ti; }
            const int tj = b - base, j = threadIdx.x, r = j >> 6, lane = j & 63;
            const int row = 16 * ti + (lane >> 4) + 4 * r, col = 16 * tj + (lane & 15);
            if (row < Rw && col < Rw) {
                const int gr = grow(row), gc = grow(col);
                if (gr >= gc) atomicAdd(&a.S[(size_t)gr * pd.D + gc], -group_sum(a.spart + (size_t)b * 256 + j));
            }
        } else {
            for (int row = threadIdx.x; row < Rw; row += blockDim.x)
                atomicAdd(&a.y[grow(row)], -group_sum(a.spart + (size_t)ntl * 256 + row));
        }
        return;
    }
    __shared__ double sB[4][36], sAd[4][36], sM[4][36], sg[4][6];
    __shared__ double sgeo[4][kPairGeomFloats];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + w;
    if (a.priv) {
        // k_edge2's private copies of y (ba_plan.hpp: kPrivY): added up, cleared, and the sum added to y
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < pd.D; i += pair_blocks * blockDim.x) {
            double s = 0.0;
            for (int c = 0; c < kPrivY; c += 8) {
                double v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = a.priv[(size_t)(c + k) * pd.D + i];
#pragma unroll
                for (int k = 0; k < 8; ++k) { s += v[k]; if (v[k] != 0.0) a.priv[(size_t)(c + k) * pd.D + i] = 0.0; }
            }
            if (s != 0.0) atomicAdd(&a.y[i], s);
        }
        // ... and its arrival counters cleared for the next step
        int *arr = reinterpret_cast<int *>(a.priv + priv_copy_doubles((size_t)pd.D, (size_t)pd.P));
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kPrivArrive; i += pair_blocks * blockDim.x) if (arr[i] != 0) arr[i] = 0;
    }
    // the tags of the dX granules, and the hand-off's time-out word: cleared for the fused solve + update launch behind this
    // kernel (ba_solve_update.hpp), whose consumers take a granule only with this step's tag on it
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < pd.D; i += pair_blocks * blockDim.x) a.dxg[i] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.status[kStatusHandoff] = 0;
    const bool live = p < pd.P;
    int ia = -1, ib = -1;
    if (live) {
        ia = pd.pair_i[p] - pd.fixedp; ib = pd.pair_j[p] - pd.fixedp;
        double *acc = a.pairacc + (size_t)p * kPairAccStride;
        double *g = sgeo[w];
        // the sums first (they need only the pair index), so their latency runs under the pose loads and the geometry
        double accv = 0.0;
        const int vi_ld = lane < 36 ? sym21(lane / 6, lane % 6) : lane < 42 ? 21 + lane - 36 : -1;
        if (pair_blocks < (int)gridDim.x) {
            // (k_etile left the tiles' sums side by side: added up here in the order of the plan's list — the list entries
            //  through the lanes, then independent loads, eight in flight)
            const int R16 = pd.max_rows16, nt = R16 >> 4;
            const size_t per_tile = sp_tile_doubles(pd.max_rows16, pd.max_tile_pairs), off = (size_t)nt * (nt + 1) / 2 * 256 + R16;
            const size_t mtp_s = (size_t)(pd.max_tile_pairs > 0 ? pd.max_tile_pairs : 1);
            const int q0 = pd.pp_ptr[p], q1 = pd.pp_ptr[p + 1];
            const double *src = a.spart + off + (size_t)(vi_ld >= 0 ? vi_ld : 0) * mtp_s;
            for (int qb = q0; qb < q1; qb += 64) {
                const int e_l = qb + lane < q1 ? pd.pp_idx[qb + lane] : 0, cnt = min(64, q1 - qb);
                for (int k0 = 0; k0 < cnt; k0 += 8) {
                    double v[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int e = __shfl(e_l, k0 + k);
                        v[k] = (k0 + k < cnt && vi_ld >= 0) ? src[(size_t)(e >> 6) * per_tile + (size_t)(e & 63)] : 0.0;      // [vi][pair] per tile
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) accv += v[k];
                }
            }
        } else if (vi_ld >= 0) {
            accv = acc[vi_ld];
            if (a.priv) {                     // ... and of the per-pair sums (kPrivP)
                double *pp = a.priv + (size_t)kPrivY * pd.D + (size_t)p * kPairAccStride + vi_ld;
                const size_t cs = (size_t)pd.P * kPairAccStride;
                double v[kPrivP];
#pragma unroll
                for (int c = 0; c < kPrivP; ++c) v[c] = pp[c * cs];
#pragma unroll
                for (int c = 0; c < kPrivP; ++c) accv += v[c];
            }
        }
        if (lane < kPairGeomFloats)                                                              // computed by the Jacobian kernel
            g[lane] = a.prec ? reinterpret_cast<const double *>(a.pairgeo)[(size_t)p * kPairGeomFloats + lane]
                             : (double)a.pairgeo[(size_t)p * kPairGeomFloats + lane];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (lane < 36) {
            const int r = lane / 6, c = lane % 6;
            sB[w][lane] = accv;
            // Ad = [[R, [t]x R], [0, R]]                                   (se3.h:58-67)
            double v = 0.0;
            if (r < 3 && c < 3) v = g[3*r + c];
            else if (r >= 3 && c >= 3) v = g[3*(r - 3) + (c - 3)];
            else if (r < 3 && c >= 3) {
                const int cc = c - 3;
                const double t0 = g[9], t1 = g[10], t2 = g[11];
                const double R0 = g[cc], R1 = g[3 + cc], R2 = g[6 + cc];
                v = r == 0 ? (-t2 * R1 + t1 * R2) : r == 1 ? (t2 * R0 - t0 * R2) : (-t1 * R0 + t0 * R1);
            }
            sAd[w][lane] = v;
        } else if (lane < 42) {
            sg[w][lane - 36] = accv;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (lane < 27 && pair_blocks == (int)gridDim.x) acc[lane] = 0.0;       // leave the per-pair sums clear for the next step
        if (a.priv && lane < 27 && pair_blocks == (int)gridDim.x) {
            double *pp = a.priv + (size_t)kPrivY * pd.D + (size_t)p * kPairAccStride + lane;
            const size_t cs = (size_t)pd.P * kPairAccStride;
#pragma unroll
            for (int c = 0; c < kPrivP; ++c) pp[c * cs] = 0.0;
        }
    }
    __syncthreads();
    if (live && lane < 36) {
        const int r = lane / 6, c = lane % 6;
        double m = 0.0;
        for (int s = 0; s < 6; ++s) m += sB[w][6*r + s] * sAd[w][6*s + c];
        sM[w][lane] = m;                                          // M = Bjj Ad
    }
    __syncthreads();
    if (!live) return;
    const int D = pd.D;
    if (lane < 36) {
        const int r = lane / 6, c = lane % 6;
        if (ia >= 0) {                                            // B[a,a] += Ad^T M
            double v = 0.0;
            for (int s = 0; s < 6; ++s) v += sAd[w][6*s + r] * sM[w][6*s + c];
            if (r >= c) atomicAdd(&a.S[(size_t)(6*ia + r) * D + 6*ia + c], v);
        }
        if (ib >= 0 && r >= c) atomicAdd(&a.S[(size_t)(6*ib + r) * D + 6*ib + c], sB[w][lane]);
        if (ia >= 0 && ib >= 0) {
            if (ia > ib)      atomicAdd(&a.S[(size_t)(6*ia + r) * D + 6*ib + c], -sM[w][6*c + r]);   // B[a,b] = -M^T
            else if (ib > ia) atomicAdd(&a.S[(size_t)(6*ib + r) * D + 6*ia + c], -sM[w][6*r + c]);   // B[b,a] = -M
            else if (r >= c)  atomicAdd(&a.S[(size_t)(6*ia + r) * D + 6*ia + c], -(sM[w][6*r + c] + sM[w][6*c + r]));
        }
    } else if (lane < 42) {
        const int c = lane - 36;
        if (ia >= 0) {
            double v = 0.0;
            for (int s = 0; s < 6; ++s) v += sAd[w][6*s + c] * sg[w][s];
            atomicAdd(&a.y[6*ia + c], -v);
        }
        if (ib >= 0) atomicAdd(&a.y[6*ib + c], sg[w][c]);
    }
}

// behind the pair blocks: the blocks that add up the tiles' Schur products of a k_etile plan with sp_ok
int launch_pair_finalize(const PlanDev &pd, const StepArgs &a, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    const int pb = (pd.P + 3) / 4, nt16 = pd.max_rows16 >> 4;
    const int sp_blocks = (pd.route.kernel == Route::kEtile && pd.sp_ok) ? pd.sg_n * (nt16 * (nt16 + 1) / 2 + 1) : 0;
    if (ev0) hipExtLaunchKernelGGL(k_pair_finalize, dim3(pb + sp_blocks), dim3(256), 0, st, ev0, ev1, 0, pd, a, pb);
    else hipLaunchKernelGGL(k_pair_finalize, dim3(pb + sp_blocks), dim3(256), 0, st, pd, a, pb);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

}  // namespace bt
