// Shared by the two FSDT kernels (fsdt.hip: element form; fsdt_st.hip: assembled-stencil form): kernel parameters and what
// FSDT does around the final reduction of the three sums of squares (dn_reduce.h).
#pragma once
#include "dn_reduce.h"

namespace dn {

struct FsdtParams {
    float b[4][4], dx[4][4], dy[4][4];     // 1-D tables at the Gauss points (derivatives scaled by 2/h)
    float w2[4][4];                        // w[jg] * w[ig] * wscale
    float D11, D12, D22, D66, A44, A55, q;
    const float* fld[3];                   // w, phi_x, phi_y
    const float* in_scale;                 // optional 3 device floats: field k is scaled as it is loaded
    const float* in_num;                   // optional 3 + 3 device floats: field k is scaled by in_num[k] / in_den[k] (0 where in_den[k] <= 0)
    const float* in_den;
    float* norms;                          // optional 3 device floats: sqrt of the three sums of squares, written by the last workgroup
    const void* mask;
    int mask_is_u8, mask_batched;
    const float* bcf[3];
    int bcf_batched[3];
    float bcv[3];
    float* out[3];
    double* part;                          // [3][nblocks] partial sums of squares
    unsigned* counter;
    double* sumsq;                         // 3 doubles
    int nx, ny, nelx, nely, rows_per_strip, want_sums, spin_limit;
    int defer_sums;                        // != 0: the launch stores its per-workgroup partials (and their count) and leaves the reduction to its consumer;
                                           // the value is the pair's ticket, left in the workspace header for the consumer to check
    int den_ticket;                        // consumer: the ticket it expects there (a mismatch -- another reducing launch used the workspace in between -- gives NaN)
    const unsigned* den_counter;           // consumer: header of the producer's workspace (DN_WS_NBLOCKS_WORD: its number of workgroups) ...
    const double* den_part;                // ... and its partials [3][nblocks]
};

// defer_sums: the workgroup's three partials and nothing else (no arrival counter, no wait: a kernel boundary orders them before the consumer)
__device__ __forceinline__ void store_partials3(const FsdtParams& p, const float (&sq)[3], int tid, int nthreads, double* red) {
    const int nblocks = launch_workgroups(), blk = workgroup_index();
    double mine[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) mine[k] = block_sum((double)sq[k], red, tid, nthreads);
    if (tid == 0) {
        double* const part[3] = {p.part, p.part + nblocks, p.part + 2 * (size_t)nblocks};
        store_partials<3, false>(part, blk, mine);
        if (blk == 0) {
            p.counter[DN_WS_NBLOCKS_WORD] = (unsigned)nblocks;
            p.counter[DN_WS_TICKET_WORD] = (unsigned)p.defer_sums;
        }
    }
}

// Consumer of a deferring launch: every workgroup forms the producer's three sums from its partials (sum_partials, then the additions of
// block_sum: the numbers finish_sums3 in dn_reduce.h gives) and returns their square roots; workgroup 0 writes the producer's sumsq / norms where asked.
// Every thread of the workgroup must call it (barriers).  Run at the start of EVERY workgroup of the consumer, so eight partials ahead
// (a load-add loop cost the B = 8 launch 29 us) and one LDS exchange for the three block sums.
__device__ __forceinline__ void den_from_partials(const FsdtParams& p, int tid, int nthreads, double* red, double* bc3, float (&den)[3]) {
    const int nb = (int)p.den_counter[DN_WS_NBLOCKS_WORD];
    const bool stale = p.den_counter[DN_WS_TICKET_WORD] != (unsigned)p.den_ticket;      // not the partials this call was paired with: never silent
    const double* const part[3] = {p.den_part, p.den_part + nb, p.den_part + 2 * (size_t)nb};
    double e3[3];
    sum_partials<3, 8, false, true>(part, nb, tid, nthreads, e3);
    const int lane = tid & (DN_WAVE - 1), wave = tid / DN_WAVE, nw = (nthreads + DN_WAVE - 1) / DN_WAVE;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double s = wave_sum(e3[k]);
        if (lane == 0) red[k * nw + wave] = s;          // red: >= 3 * nthreads / 64 doubles
    }
    __syncthreads();
    if (tid == 0) {
        const bool first = blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double e = 0.0;
            for (int w = 0; w < nw; ++w) e += red[k * nw + w];
            bc3[k] = e;
            if (first) {
                if (p.sumsq) p.sumsq[k] = stale ? __builtin_nan("") : e;
                if (p.norms) p.norms[k] = stale ? __builtin_nanf("") : (float)sqrt(e);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) den[k] = stale ? __builtin_nanf("") : (float)sqrt(bc3[k]);
}

// fsdt_st.hip: the assembled-stencil form
int fsdt_st_launch(const dn_mesh* m, float wscale, FsdtParams& pp, hipStream_t s);
int64_t fsdt_st_workgroups(const dn_mesh* m);

}  // namespace dn
