// The deterministic final reduction every fused operator ends with, once: the layout of a workspace header, the arrival of a
// workgroup, the fixed-order sum of N arrays of per-workgroup partials and the store of a workgroup's own partials.  What Poisson
// and FSDT do with the totals stays in poisson_common.h and fsdt_common.h.
//
// Every workgroup leaves its fp64 partial sums in the workspace and arrives at a counter; the workgroup that arrives last adds all
// partials in index order (=> the same sums whatever the arrival order) and resets the counters, so the workspace is ready for the
// next launch.  Two-level arrival (DN_NSHARD shard counters on separate 64-B lines, then one top counter) keeps the same-address
// atomic fan-in at ~nblocks/64 + 64 instead of nblocks (one address retires only ~88 atomics/us: MI355X_MICROARCH.md "fanin").
// Visibility (cdna_hip_programming.md, Guideline 16): thread 0 stores its partials write-through (sc1: relaxed agent-scope atomic
// stores) and drains them before the arrival atomic, instead of an agent-scope release fence -- a release is a `buffer_wbl2` of the
// whole XCD L2, i.e. every workgroup would wait for everybody's freshly written output lines to be flushed (measured: +5..30 us per
// workgroup at 8k workgroups).  All arrival atomics are relaxed; only the last arriver acquires (agent scope, thread 0, then a
// barrier) and it reads the partials with sc1 loads.
#pragma once
#include "dn_common.h"

namespace dn {

// Workspace header: the top counter's 64-B line, then DN_NSHARD shard counters on a line each; the partials lie behind it.
constexpr int DN_NSHARD = 64;
constexpr int DN_WS_SHARD_STRIDE = 16;                    // words between counters (one 64-B line each)
static constexpr int64_t DN_WS_HEADER = 64 * (1 + 64);
static_assert(DN_WS_HEADER == (int64_t)sizeof(unsigned) * DN_WS_SHARD_STRIDE * (1 + DN_NSHARD), "header = top line + shard lines");
// further words of the top counter's line
constexpr int DN_WS_NBLOCKS_WORD = 4;      // a launch that defers its reduction to a consumer launch leaves its number of workgroups here ...
constexpr int DN_WS_TICKET_WORD = 5;       // ... and the pair's ticket here (0 after any launch that reduced in the kernel)
constexpr int DN_WS_ERRWORD = 8;           // sticky error bits of the launches that used this workspace (bit 0: a bounded LDS hand-over poll of a
                                           // chained-strip kernel ran out -- its results are NaN); read and cleared by dn_workspace_status

__device__ __forceinline__ int launch_workgroups() { return gridDim.x * gridDim.y * gridDim.z; }
__device__ __forceinline__ int workgroup_index() { return (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; }

// Thread 0 stores its workgroup's N partials.  PUBLISH: to the last arriver of the same launch (write-through and drained: the arrival
// atomic may follow); otherwise plain stores, which the kernel boundary orders before their reader.
template <int N, bool PUBLISH>
__device__ __forceinline__ void store_partials(double* const (&part)[N], int blk, const double (&v)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if constexpr (PUBLISH) __hip_atomic_store(&part[k][blk], v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else part[k][blk] = v[k];
    }
    if constexpr (PUBLISH) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Arrival of workgroup blk of nblocks (thread 0, after store_partials<N, true>): true for the workgroup that arrives last.  Shard counters
// are reset by their last arriver, the top counter by arrival_reset.  SINGLE_UP_TO_NSHARD: launches of at most DN_NSHARD workgroups arrive
// at the top counter alone (one atomic round trip on the launch's critical path instead of two).
template <bool SINGLE_UP_TO_NSHARD>
__device__ __forceinline__ bool arrive_last(unsigned* counter, int nblocks, int blk) {
    if (SINGLE_UP_TO_NSHARD && nblocks <= DN_NSHARD)
        return __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(nblocks - 1);
    const int nshard = SINGLE_UP_TO_NSHARD ? DN_NSHARD : (nblocks < DN_NSHARD ? nblocks : DN_NSHARD);
    const int shard = blk % nshard;
    const unsigned in_shard = (unsigned)((nblocks - shard + nshard - 1) / nshard);
    unsigned* sc = counter + DN_WS_SHARD_STRIDE * (1 + shard);
    if (__hip_atomic_fetch_add(sc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != in_shard - 1) return false;
    __hip_atomic_store(sc, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(nshard - 1);
}

// ... by thread 0 of the last arriver, once it has written the totals
__device__ __forceinline__ void arrival_reset(unsigned* counter) {
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Fixed-order sum of N arrays of n partials: thread t adds partials t, t + nthreads, ... of each array in turn; the caller's fixed-order
// block sum follows.  AHEAD partials of each array are requested before the first is added (one memory round trip per AHEAD instead of per
// partial: the loop of a last arriver is the critical path of its whole launch); the order of additions, and so every bit of the
// sums, does not depend on AHEAD.  SC1: agent-scope loads, for partials stored by the same launch; plain loads across a kernel boundary.
// BY_ARRAY: the order of the requests -- array by array, or partial by partial across the arrays.  It changes no number, only the code
// around the loop: each family keeps the order its kernels were tuned with (profiles/reduce_refactor.txt: registers of the FSDT / flow
// kernels with one order, 0.07 us of the 64^2 Poisson launch with the other).
template <int N, int AHEAD, bool SC1, bool BY_ARRAY, class T>       // T: double or const double
__device__ __forceinline__ void sum_partials(T* const (&part)[N], int n, int tid, int nthreads, double (&acc)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    for (int i0 = tid; i0 < n; i0 += nthreads * AHEAD) {
        double v[N][AHEAD];
#pragma unroll
        for (int q = 0; q < N * AHEAD; ++q) {
            const int k = BY_ARRAY ? q / AHEAD : q % N, j = BY_ARRAY ? q % AHEAD : q / N;
            const int i = i0 + j * nthreads;
            const int ic = i < n ? i : 0;
            if constexpr (SC1) v[k][j] = __hip_atomic_load(&part[k][ic], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else v[k][j] = part[k][ic];
        }
#pragma unroll
        for (int q = 0; q < N * AHEAD; ++q) {
            const int k = BY_ARRAY ? q / AHEAD : q % N, j = BY_ARRAY ? q % AHEAD : q / N;
            acc[k] += (i0 + j * nthreads < n) ? v[k][j] : 0.0;
        }
    }
}

// The in-launch reduction from the workgroup's own sums (mine: valid in thread 0) to the per-thread sums of the last arriver: true in
// every thread of the workgroup that arrived last, which then block-sums acc, writes the totals and calls arrival_reset.  Every thread of
// the workgroup must call it (barriers); flag: one int of LDS.
template <int N, int AHEAD, bool SINGLE_UP_TO_NSHARD, bool BY_ARRAY>
__device__ __forceinline__ bool last_arriver_sums(double* const (&part)[N], unsigned* counter, const double (&mine)[N], int tid, int nthreads,
                                                  int* flag, double (&acc)[N]) {
    const int nblocks = launch_workgroups();
    if (tid == 0) {
        const int blk = workgroup_index();
        store_partials<N, true>(part, blk, mine);
        *flag = arrive_last<SINGLE_UP_TO_NSHARD>(counter, nblocks, blk) ? 1 : 0;
    }
    __syncthreads();
    if (!*flag) return false;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    sum_partials<N, AHEAD, true, BY_ARRAY>(part, nblocks, tid, nthreads, acc);
    return true;
}

// The tail of the operators that reduce N sums of squares (part: [N][nblocks]): block sums, the in-launch reduction, sumsq and
// norms = sqrt where asked, and the ticket of an earlier deferring launch in this workspace is cleared (its partials are gone).
// red: >= nthreads / 64 doubles.
template <int N>
__device__ __forceinline__ void finish_sums(double* part, unsigned* counter, double* sumsq, float* norms, const float (&sq)[N], int tid,
                                            int nthreads, double* red, int* flag) {
    const int nblocks = launch_workgroups();
    double* parts[N];
#pragma unroll
    for (int k = 0; k < N; ++k) parts[k] = part + k * (size_t)nblocks;
    double mine[N], tot[N];
#pragma unroll
    for (int k = 0; k < N; ++k) mine[k] = block_sum((double)sq[k], red, tid, nthreads);
    if (!last_arriver_sums<N, 8, false, true>(parts, counter, mine, tid, nthreads, flag, tot)) return;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double e = block_sum(tot[k], red, tid, nthreads);
        if (tid == 0) {
            if (sumsq) sumsq[k] = e;
            if (norms) norms[k] = (float)sqrt(e);
        }
    }
    if (tid == 0) {
        arrival_reset(counter);
        counter[DN_WS_TICKET_WORD] = 0u;
    }
}

// ... three of them (FSDT, Stokes, Navier-Stokes)
__device__ __forceinline__ void finish_sums3(double* part, unsigned* counter, double* sumsq, float* norms, const float (&sq)[3], int tid,
                                             int nthreads, double* red, int* flag) {
    finish_sums<3>(part, counter, sumsq, norms, sq, tid, nthreads, red, flag);
}

}  // namespace dn
