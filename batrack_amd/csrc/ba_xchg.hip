// ba_xchg.hip — the multi-GPU exchange form of the reduced system: [S | y] <-> its packed non-zero blocks, and the one-shot
// peer-write exchange of the packed form between the ranks' GPUs (gfx950).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "ba_kernels.hpp"

namespace bt {

// ------------------------------------------------------------------ k_pack_system
// Dense [S | y] (caller order, lower triangle) <-> the plan's non-zero blocks in factor order followed by
// y in factor order: the multi-GPU exchange buffer (include/batrack_ba.h: bt_ba_pack).  One thread per element.
// block b of a WIDE plan's packed form (ba_plan_solver.cpp: no symbolic factorisation, every lower block): b = rn (rn + 1) / 2 + cn
__device__ __forceinline__ void wide_block(int b, int &rn, int &cn) {
    rn = (int)((sqrtf(8.0f * (float)b + 1.0f) - 1.0f) * 0.5f);
    while ((rn + 1) * (rn + 2) / 2 <= b) ++rn;
    while (rn * (rn + 1) / 2 > b) --rn;
    cn = b - rn * (rn + 1) / 2;
}

template <bool UNPACK>
__global__ __launch_bounds__(256) void k_pack_system(PlanDev pd, StepArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, nb = pd.nnzb * 36;
    if (pd.wide) {
        if (i < nb) {
            const int b = i / 36, e = i - 36 * b, r = e / 6, c = e - 6 * r;
            int rn, cn;
            wide_block(b, rn, cn);
            if (rn == cn && c > r) { if (!UNPACK) a.packed[i] = 0.0; return; }
            double *p = a.S + (size_t)(6 * rn + r) * pd.D + 6 * cn + c;
            if (UNPACK) *p = a.packed[i]; else a.packed[i] = *p;
        } else if (i < nb + pd.D) {
            if (UNPACK) a.y[i - nb] = a.packed[i]; else a.packed[i] = a.y[i - nb];
        }
        return;
    }
    if (i < nb) {
        const int b = i / 36, e = i - 36 * b, r = e / 6, c = e - 6 * r, src = pd.blk_src[b];
        const int rn = src >> 9, cn = (src >> 1) & 255;
        const bool diag = rn == cn;
        if (diag && c > r) { if (!UNPACK) a.packed[i] = 0.0; return; }       // S holds the lower triangle only
        double *p = (src & 1) ? a.S + (size_t)(6 * rn + c) * pd.D + 6 * cn + r : a.S + (size_t)(6 * rn + r) * pd.D + 6 * cn + c;
        if (UNPACK) *p = a.packed[i]; else a.packed[i] = *p;
    } else if (i < nb + pd.D) {
        const int k = i - nb;
        double *p = a.y + 6 * pd.perm[k / 6] + k % 6;
        if (UNPACK) *p = a.packed[i]; else a.packed[i] = *p;
    }
}

// ------------------------------------------------------------------ one-shot exchange of [S | y] between the ranks' GPUs
// The reduced system in its packed form is ~140 KB at 64 keyframes, ~33 KB for the 15-pose window: an all-reduce of that
// size is pure latency, and xGMI is a full mesh of point-to-point links — so every rank WRITES its packed partial system
// straight into a slot of every peer's exchange buffer (hipIpc-mapped, uncached device memory) and raises a flag there;
// every rank then sums the `world` slots of its own buffer in rank order (bitwise the same sum everywhere, so every rank
// solves the identical system) while unpacking into [S | y].  No collective library, no host round trip, nothing but two
// kernels on the compute stream.  Buffer layout (bt_xchg_bytes): [2 parities][world slots][slot doubles] | flags [2][world]
// int64 | a ticket counter.  Epoch e uses parity e & 1: a rank cannot start epoch e + 2 before it has seen every peer's flag
// of epoch e + 1, which a peer raises only after it has consumed epoch e.
__device__ __forceinline__ double *packed_elem(const PlanDev &pd, const StepArgs &a, int i, bool &zero) {
    const int nb = pd.nnzb * 36;
    zero = false;
    if (pd.wide) {
        if (i >= nb) return a.y + (i - nb);
        const int b = i / 36, e = i - 36 * b, r = e / 6, c = e - 6 * r;
        int rn, cn;
        wide_block(b, rn, cn);
        if (rn == cn && c > r) { zero = true; return nullptr; }
        return a.S + (size_t)(6 * rn + r) * pd.D + 6 * cn + c;
    }
    if (i < nb) {
        const int b = i / 36, e = i - 36 * b, r = e / 6, c = e - 6 * r, src = pd.blk_src[b];
        const int rn = src >> 9, cn = (src >> 1) & 255;
        if (rn == cn && c > r) { zero = true; return nullptr; }              // S holds the lower triangle only
        return (src & 1) ? a.S + (size_t)(6 * rn + c) * pd.D + 6 * cn + r : a.S + (size_t)(6 * rn + r) * pd.D + 6 * cn + c;
    }
    const int k = i - nb;
    return a.y + 6 * pd.perm[k / 6] + k % 6;
}

struct XchgPeers { double *buf[kMaxRanks]; };

__device__ __forceinline__ size_t xchg_slot_doubles(const PlanDev &pd) { return ((size_t)pd.nnzb * 36 + pd.D + 1) & ~(size_t)1; }

__global__ __launch_bounds__(256) void k_xchg_push(PlanDev pd, StepArgs a, XchgPeers peers, int world, int rank, long long epoch) {
    const int total = pd.nnzb * 36 + pd.D;
    const size_t slot = xchg_slot_doubles(pd), off = ((size_t)(epoch & 1) * world + rank) * slot;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        bool zero;
        double *p = packed_elem(pd, a, i, zero);
        const double v = zero ? 0.0 : *p;
        for (int q = 0; q < world; ++q) __builtin_nontemporal_store(v, peers.buf[q] + off + i);
    }
    // every block: its stores out to the fabric, then a ticket; the last block raises this rank's flag in every peer's buffer
    __threadfence_system();
    __syncthreads();
    __shared__ int last;
    long long *own_flags = reinterpret_cast<long long *>(peers.buf[rank] + 2 * (size_t)world * slot);
    int *ticket = reinterpret_cast<int *>(own_flags + 2 * world);
    if (threadIdx.x == 0) last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence_system();
    if ((int)threadIdx.x < world) {
        long long *f = reinterpret_cast<long long *>(peers.buf[threadIdx.x] + 2 * (size_t)world * slot) + (size_t)(epoch & 1) * world + rank;
        __hip_atomic_store(f, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Waits for the flags of epoch `epoch` from all ranks, then [S | y] = sum over the ranks' slots, in rank order.  The wait is
// bounded (a peer that never arrives must not hang the GPU).  A time-out is FATAL for the step, never a silent wrong answer:
// status word 1 is set to BT_XCHG_TIMEOUT (sticky until bt_ba_workspace_init), and the last block to finish plants a
// non-positive pivot in S, so that the solver that follows reports a failed factorisation and the step leaves the poses
// where they were (dX = 0, the reference's own reaction to a failed Cholesky, ba.py:9-13) instead of solving a partial system;
// the depths then move by their rank-local Q w' only.  The caller polls bt_ba_xchg_status and raises (parallel.py).
__global__ __launch_bounds__(256) void k_xchg_pull(PlanDev pd, StepArgs a, double *own, int world, long long epoch, long long spin_limit) {
    const size_t slot = xchg_slot_doubles(pd);
    const long long *flags = reinterpret_cast<const long long *>(own + 2 * (size_t)world * slot) + (size_t)(epoch & 1) * world;
    if ((int)threadIdx.x < world) {
        long long it = 0;
        while (__hip_atomic_load(flags + threadIdx.x, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < epoch) {
            __builtin_amdgcn_s_sleep(8);
            if (++it > spin_limit) { __hip_atomic_store(a.status + 1, (int)BT_XCHG_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
        }
    }
    __syncthreads();
    __threadfence_system();
    const int total = pd.nnzb * 36 + pd.D;
    const double *base = own + (size_t)(epoch & 1) * world * slot;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        bool zero;
        double *p = packed_elem(pd, a, i, zero);
        if (zero) continue;
        double v = 0.0;
        for (int q = 0; q < world; ++q) v += __builtin_nontemporal_load(base + (size_t)q * slot + i);
        *p = v;
    }
    // the last block (a ticket in the rank's own buffer: the push of this step left it at 0) checks the verdict of ALL blocks
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        long long *own_flags = reinterpret_cast<long long *>(own + 2 * (size_t)world * slot);
        int *ticket = reinterpret_cast<int *>(own_flags + 2 * world) + 1;
        if (__hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1) {
            __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__hip_atomic_load(a.status + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)BT_XCHG_TIMEOUT)
                for (int d = 0; d < pd.D; ++d) a.S[(size_t)d * pd.D + d] = -1e300;      // every pivot fails whatever the elimination order
        }
    }
}

size_t xchg_bytes(const PlanDev &pd, int world) {
    const size_t slot = (((size_t)pd.nnzb * 36 + pd.D + 1) & ~(size_t)1) * sizeof(double);
    return 2 * (size_t)world * slot + 2 * (size_t)world * sizeof(long long) + 64;
}

int launch_xchg_push(const PlanDev &pd, const StepArgs &a, void *const *bufs, int world, int rank, long long epoch, hipStream_t st) {
    const int total = pd.nnzb * 36 + pd.D;
    if (total <= 0) return BT_OK;
    XchgPeers P{};
    for (int q = 0; q < world; ++q) P.buf[q] = static_cast<double *>(bufs[q]);
    const int nb = std::min(64, (total + 255) / 256);
    hipLaunchKernelGGL(k_xchg_push, dim3(nb), dim3(256), 0, st, pd, a, P, world, rank, epoch);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

int launch_xchg_pull(const PlanDev &pd, const StepArgs &a, void *own, int world, long long epoch, hipStream_t st) {
    const int total = pd.nnzb * 36 + pd.D;
    if (total <= 0) return BT_OK;
    static const long long limit = std::getenv("BT_XCHG_SPIN_LIMIT") ? std::atoll(std::getenv("BT_XCHG_SPIN_LIMIT")) : 20000000ll;   // tens of seconds of polls (each an uncached load + s_sleep): first-launch code loading and host stalls must not trip it
    const int nb = std::min(64, (total + 255) / 256);
    hipLaunchKernelGGL(k_xchg_pull, dim3(nb), dim3(256), 0, st, pd, a, static_cast<double *>(own), world, epoch, limit);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

int launch_pack(const PlanDev &pd, const StepArgs &a, bool unpack, hipStream_t st) {
    const int total = pd.nnzb * 36 + pd.D;
    if (total <= 0) return BT_OK;
    if (unpack) hipLaunchKernelGGL(k_pack_system<true>, dim3((total + 255) / 256), dim3(256), 0, st, pd, a);
    else        hipLaunchKernelGGL(k_pack_system<false>, dim3((total + 255) / 256), dim3(256), 0, st, pd, a);
    return hipGetLastError() == hipSuccess ? BT_OK : BT_EHIP;
}

}  // namespace bt
