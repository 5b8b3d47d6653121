// The vector side of a batched, matrix-free, Jacobi-preconditioned conjugate-gradient solve of the Q1 Poisson problem
// Z (K_nu u~ - F f) = 0: dn_poisson_diag and dn_poisson_cg (include/diffnet_hip.h).  The operator launch q = Z K p of an iteration is
// dn_poisson_apply itself (alpha = 1, f absent, homogeneous conditions); what was missing is below.
//
// dn_poisson_diag -- the inverse diagonal of K_nu in one launch, no workspace:
//     diag_a = wscale sum_{e contains a} sum_g gpw_g nu_g |grad N_a(g)|^2,     nu_g = sum_b N_b(g) nu_b  (the operator's interpolation)
//     dinv_a = 0 on a Dirichlet node and where diag_a == 0 (a node surrounded by nu = 0 carries no equation), 1 / diag_a elsewhere.
// The plain form in 2-D and 3-D: one thread per node gathers the nu values around it once and adds the contributions of its <= 2^nsd
// elements in the fixed order (z, y, x).  A row-marching 2-D form does not come cheaply from q1_owner_march.h (its hand-over carries the
// four element-local contributions of TWO outputs; a third march body for a launch that runs once per solve is not worth its code), so
// the plain form serves both dimensions.  Because nu_g is multilinear in the nodal values, the Gauss sum of an element factorises:
//     sum_g w_g nu_g |grad N_a|^2 = sum_b nu_b ( D_x[ax][bx] M_y[ay][by] M_z[az][bz] + M_x D_y M_z + M_x M_y D_z )
// with the 1-D tables M[a][b] = sum_g w_g N_b(g) N_a(g)^2 and D[a][b] = sum_g w_g N_b(g) (N_a'(g) 2/h)^2, formed on the host in double
// for whichever rule (2..4 points) the mesh carries: 8 x 8 multiply-adds per node in 3-D, no Gauss loop in the kernel, one instantiation
// for all rules.  Every node is written once, by its own thread, with additions in an order that depends on nothing but the node: the
// output is bitwise reproducible and bitwise independent of the batch size.
//
// dn_poisson_cg -- the vector phases of one PCG iteration, each ONE launch over flat per-sample arrays of n floats (sample b at element
// b n).  Per-sample scalars live in a 64-byte device block (dn_cg_state); no phase needs the host.
//     INIT       r = -out, p = dinv r, rz = sum r (dinv r), rr0 = rr = sum r r, active = rr0 > atol^2, iterations = 0, flags = 0
//     DOT        pq = sum p q;  alpha = rz / pq if active and pq > 0, else 0 (an active sample with !(pq > 0): BREAKDOWN, active = 0)
//     UPDATE     x += alpha p, r -= alpha q, rz' = sum r (dinv r), rr = sum r r;  beta = rz' / rz, rz = rz', iterations += 1,
//                active = rr > max(tol^2 rr0, atol^2)
//     DIRECTION  p = dinv r + beta p
// Floats moved per node and iteration: DOT 2 (p, q), UPDATE 7 (x, p, r, q, dinv read; x, r written), DIRECTION 4 (dinv, r, p read; p
// written) = 13, beside the operator launch.  (The single-reduction Chronopoulos-Gear arrangement would save one launch and the DOT pass
// but needs s = K (dinv r) recurrences whose rounding drifts from the true residual; the textbook arrangement is the one the float64
// restatement in tests/solve_ref.py mirrors line by line.)
// Inactive samples: a workgroup of an inactive sample reads none of its arrays and writes none -- x, r, p stay bitwise as they are even
// when p or q hold NaN --, it contributes zeros to the partial sums and its scalars are left alone (DOT sets its alpha to 0).
// Dot products: float64 sums of products of the float32 values.  A sample is cut into G = ceil(n / chunk) chunks (chunk a multiple of 1024
// that depends on n alone), one workgroup of 256 threads per chunk and sample; a thread owns the quads 4 (t + 256 k) .. + 3 of its chunk
// IN SAMPLE coordinates and adds their products in that order, so neither the batch size, nor a sample's position in the batch, nor the
// alignment of its base changes an addition.  Workgroup sums go to the workspace (write-through, drained), workgroups arrive at their
// SAMPLE's counters (the scheme of dn_reduce.h, one header per sample; no agent-scope release), and the sample's last arriver adds its G
// partials in a fixed order -- thread t takes partials t, t + 256, ..., then the block sum -- and updates the sample's scalars:
// reproducible run to run, independent of B and of which samples are active, and the tails of a batch's samples run side by side (a
// first version let the launch's last workgroup finish all samples one after the other: 10 us of serial tail at B = 16).  The workspace
// is zero-filled once and resets itself.
// Accesses: 16 bytes per lane in the body.  A sample's base is only 4-byte aligned when n is odd; the quads are then read and written as
// 4-byte-aligned dwordx4 accesses (the hardware takes them; as in the closed-form kernel's rows of 4 k + 1 nodes), the last < 4 nodes of a
// sample one by one.  At n = 512^2, B = 1 the launch has 256 workgroups (one per CU); the chunk grows only past 2048 workgroups a sample.
//
// dn_poisson_pcg -- the same template for a preconditioner that is a PROCEDURE (z = M r from a multigrid V-cycle, csrc/poisson_mg.hip)
// rather than a diagonal: the phases above form dinv r inline, these read z from memory.
//     RESID0     r = -out, rr0 = rr = sum r r, rz = 0, active = rr0 > atol^2, iterations = 0, flags = 0
//     UPDATE     x += alpha p, r -= alpha q, rr = sum r r, iterations += 1, active = rr > max(tol^2 rr0, atol^2), a NaN rr: BREAKDOWN
//     RZ         rz' = sum r z, beta = rz' / rz (0 where rz is not positive: the first call after RESID0), rz = rz'
//     DIRECTION  p = z + beta p (p = z where beta == 0: the first direction does not depend on what p held)
// between them: the V-cycle on r, and dn_poisson_cg's DOT unchanged.  One sum per phase; the same state block, workspace, chunks,
// reduction and inactive-sample rule.  Floats per node and iteration beside the operator and the V-cycle: DOT 2, UPDATE 6, RZ 2,
// DIRECTION 3.
#include "dn_reduce.h"

namespace dn {

struct __attribute__((packed, aligned(4))) F4U { float v[4]; };

struct CgState {
    double rz, rr, rr0, pq;
    float alpha, beta;
    int32_t active, iterations, flags;
    int32_t pad[3];
};
static_assert(sizeof(CgState) == sizeof(dn_cg_state), "dn_cg_state is the device block");
static_assert(sizeof(CgState) == 64, "one 64-byte line per sample");

constexpr int CG_THREADS = 256;
constexpr int CG_QUANTUM = 4 * CG_THREADS;        // nodes one pass of a workgroup covers
constexpr int CG_MAX_CHUNKS = 2048;               // workgroups per sample before the chunk grows

static inline void cg_geometry(int64_t n, int& chunk, int& G) {
    const int64_t mult = std::max<int64_t>(1, (n + (int64_t)CG_QUANTUM * CG_MAX_CHUNKS - 1) / ((int64_t)CG_QUANTUM * CG_MAX_CHUNKS));
    chunk = (int)(mult * CG_QUANTUM);
    G = (int)((n + chunk - 1) / chunk);
}

// ---- the inverse diagonal ----------------------------------------------------------------------------------------------------------
struct DiagParams {
    const float* nu;
    int nu_batched;
    const void* mask[2];
    int mask_kind[2];                      // 0 absent, 1 uint8, 2 fp32
    int mask_batched[2];
    float* dinv;
    float M[3][2][2], D[3][2][2];          // [axis x, y, z][a][b]
    float wscale;
    int unit;
    int nx, ny, nz;
};

template <int NSD>
__global__ void __launch_bounds__(64) poisson_diag_kernel(const DiagParams p) {
    constexpr int EZ = NSD == 3 ? 2 : 1, NZ = NSD == 3 ? 3 : 1;
    const int nx = p.nx, ny = p.ny, nz = p.nz;
    const int cx = (nx + 63) >> 6;
    const int i = ((int)blockIdx.x % cx) * 64 + (int)threadIdx.x;
    const int j = (int)blockIdx.x / cx, k = (int)blockIdx.y;
    const int b = blockIdx.z;
    const bool live = i < nx;
    const int64_t nps = (int64_t)nx * ny * nz;

    // the nu values around the node (indices clamped into the mesh: a clamped value only feeds an element that does not exist)
    float NU[NZ][3][3];
    const float* nub = p.nu ? p.nu + (p.nu_batched ? (int64_t)b * nps : 0) : nullptr;
#pragma unroll
    for (int dz = 0; dz < NZ; ++dz)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int kk = NSD == 3 ? min(max(k + dz - 1, 0), nz - 1) : 0;
                const unsigned off = ((unsigned)kk * (unsigned)ny + (unsigned)min(max(j + dy - 1, 0), ny - 1)) * (unsigned)nx +
                                     (unsigned)min(max(i + dx - 1, 0), nx - 1);
                NU[dz][dy][dx] = nub ? ld_at<float>(nub, off) : 1.f;
            }

    float acc = 0.f;
    // the node's elements in the fixed order z, y, x; in element (k + ez - 1, j + ey - 1, i + ex - 1) the node is local node (1 - ez, 1 - ey, 1 - ex)
#pragma unroll
    for (int ez = 0; ez < EZ; ++ez)
#pragma unroll
        for (int ey = 0; ey < 2; ++ey)
#pragma unroll
            for (int ex = 0; ex < 2; ++ex) {
                bool ok = (i + ex - 1) >= 0 && (i + ex - 1) < nx - 1 && (j + ey - 1) >= 0 && (j + ey - 1) < ny - 1;
                if constexpr (NSD == 3) ok = ok && (k + ez - 1) >= 0 && (k + ez - 1) < nz - 1;
                const int ax = 1 - ex, ay = 1 - ey, az = 1 - ez;
                float e = 0.f;
#pragma unroll
                for (int bz = 0; bz < EZ; ++bz)
#pragma unroll
                    for (int by = 0; by < 2; ++by)
#pragma unroll
                        for (int bx = 0; bx < 2; ++bx) {
                            const float mx = p.M[0][ax][bx], dx = p.D[0][ax][bx], my = p.M[1][ay][by], dy = p.D[1][ay][by];
                            float t;
                            if constexpr (NSD == 3) {
                                const float mz = p.M[2][az][bz], dz = p.D[2][az][bz];
                                t = fmaf(dx * my, mz, fmaf(mx * dy, mz, (mx * my) * dz));
                            } else {
                                t = fmaf(dx, my, mx * dy);
                            }
                            e = fmaf(NU[ez + bz][ey + by][ex + bx], t, e);
                        }
                acc += ok ? e : 0.f;
            }
    const float diag = p.wscale * acc;

    if (!live) return;
    const unsigned off = ((unsigned)k * (unsigned)ny + (unsigned)j) * (unsigned)nx + (unsigned)i;
    bool fixed = false;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (p.mask_kind[c] == 0) continue;
        const int64_t mo = p.mask_batched[c] ? (int64_t)b * nps : 0;
        if (p.mask_kind[c] == 1) fixed = fixed || ld_at<uint8_t>(reinterpret_cast<const uint8_t*>(p.mask[c]) + mo, off) != 0;
        else fixed = fixed || ld_at<float>(reinterpret_cast<const float*>(p.mask[c]) + mo, off) > 0.5f;
    }
    const float inv = p.unit ? 1.f : 1.f / diag;
    st_at<float>(p.dinv + (int64_t)b * nps, off, (fixed || diag == 0.f) ? 0.f : inv);
}

// ---- the vector phases -------------------------------------------------------------------------------------------------------------
struct CgParams {
    float* x;
    float* r;
    float* p;
    const float* q;
    const float* dinv;
    const float* z;                        // the dn_poisson_pcg phases: the preconditioned residual
    int dinv_batched;
    CgState* st;
    unsigned* counter;
    double* part;                          // [2][G * batch]
    unsigned n;
    int chunk, G, batch;
    float tol, atol;
};

// phases of dn_poisson_pcg as values of the same template parameter
constexpr int PCG_RESID0 = 4, PCG_UPDATE = 5, PCG_RZ = 6, PCG_DIRECTION = 7;

template <int PHASE>
__global__ void __launch_bounds__(CG_THREADS) poisson_cg_kernel(const CgParams p) {
    constexpr int NS = (PHASE == DN_CG_DOT || PHASE >= PCG_RESID0) ? 1 : 2;            // sums of the phase (DIRECTION: none)
    const int tid = threadIdx.x, g = blockIdx.x, b = blockIdx.y;
    __shared__ double red[2 * CG_THREADS / DN_WAVE];
    __shared__ int flag;

    CgState* stb = p.st + b;
    const bool act = (PHASE == DN_CG_INIT || PHASE == PCG_RESID0) ? true : stb->active != 0;
    const float alpha = (PHASE == DN_CG_UPDATE || PHASE == PCG_UPDATE) ? stb->alpha : 0.f;
    const float beta = (PHASE == DN_CG_DIRECTION || PHASE == PCG_DIRECTION) ? stb->beta : 0.f;
    double s0 = 0.0, s1 = 0.0;

    if (act) {
        const int64_t base = (int64_t)b * p.n;
        float* xb = p.x + base;
        float* rb = p.r + base;
        float* pb = p.p + base;
        const float* qb = p.q + base;
        const float* db = PHASE >= PCG_RESID0 ? p.z + base : p.dinv + (p.dinv_batched ? base : 0);      // the pcg phases read z in dinv's place
        const unsigned c0 = (unsigned)g * (unsigned)p.chunk, c1 = min(c0 + (unsigned)p.chunk, p.n);

        // one node of the phase: the same arithmetic in the quads and in the tail
        auto node = [&](float& xv, float& rv, float& pv, float qv, float dv) {
            if constexpr (PHASE == DN_CG_INIT) {
                rv = -qv;
                pv = dv * rv;
                s0 += (double)rv * (double)pv;
                s1 += (double)rv * (double)rv;
            } else if constexpr (PHASE == DN_CG_DOT) {
                s0 += (double)pv * (double)qv;
            } else if constexpr (PHASE == DN_CG_UPDATE) {
                xv = fmaf(alpha, pv, xv);
                rv = fmaf(-alpha, qv, rv);
                const float zv = dv * rv;
                s0 += (double)rv * (double)zv;
                s1 += (double)rv * (double)rv;
            } else if constexpr (PHASE == DN_CG_DIRECTION) {
                pv = fmaf(beta, pv, dv * rv);
            } else if constexpr (PHASE == PCG_RESID0) {
                rv = -qv;
                s0 += (double)rv * (double)rv;
            } else if constexpr (PHASE == PCG_UPDATE) {
                xv = fmaf(alpha, pv, xv);
                rv = fmaf(-alpha, qv, rv);
                s0 += (double)rv * (double)rv;
            } else if constexpr (PHASE == PCG_RZ) {
                s0 += (double)rv * (double)dv;
            } else {
                pv = beta == 0.f ? dv : fmaf(beta, pv, dv);
            }
        };
        constexpr bool RX = PHASE == DN_CG_UPDATE || PHASE == PCG_UPDATE, WX = RX;
        constexpr bool RR = RX || PHASE == DN_CG_DIRECTION || PHASE == PCG_RZ, WR = PHASE == DN_CG_INIT || PHASE == PCG_RESID0 || RX;
        constexpr bool RP = PHASE != DN_CG_INIT && PHASE != PCG_RESID0 && PHASE != PCG_RZ;
        constexpr bool WP = PHASE == DN_CG_INIT || PHASE == DN_CG_DIRECTION || PHASE == PCG_DIRECTION;
        constexpr bool RQ = PHASE != DN_CG_DIRECTION && PHASE != PCG_RZ && PHASE != PCG_DIRECTION;
        constexpr bool RD = PHASE != DN_CG_DOT && PHASE != PCG_RESID0 && PHASE != PCG_UPDATE;      // dinv, or z in the pcg phases

        for (unsigned i = c0 + 4u * (unsigned)tid; i < c1; i += CG_QUANTUM) {
            if (i + 4u <= c1) {
                F4U xv = {}, rv = {}, pv = {}, qv = {}, dv = {};
                if constexpr (RX) xv = ld_at<F4U>(xb, i);
                if constexpr (RR) rv = ld_at<F4U>(rb, i);
                if constexpr (RP) pv = ld_at<F4U>(pb, i);
                if constexpr (RQ) qv = ld_at<F4U>(qb, i);
                if constexpr (RD) dv = ld_at<F4U>(db, i);
#pragma unroll
                for (int c = 0; c < 4; ++c) node(xv.v[c], rv.v[c], pv.v[c], qv.v[c], dv.v[c]);
                if constexpr (WX) st_at<F4U>(xb, i, xv);
                if constexpr (WR) st_at<F4U>(rb, i, rv);
                if constexpr (WP) st_at<F4U>(pb, i, pv);
            } else {
                for (unsigned e = i; e < c1; ++e) {               // the last < 4 nodes of the sample
                    float xv = 0.f, rv = 0.f, pv = 0.f, qv = 0.f, dv = 0.f;
                    if constexpr (RX) xv = ld_at<float>(xb, e);
                    if constexpr (RR) rv = ld_at<float>(rb, e);
                    if constexpr (RP) pv = ld_at<float>(pb, e);
                    if constexpr (RQ) qv = ld_at<float>(qb, e);
                    if constexpr (RD) dv = ld_at<float>(db, e);
                    node(xv, rv, pv, qv, dv);
                    if constexpr (WX) st_at<float>(xb, e, xv);
                    if constexpr (WR) st_at<float>(rb, e, rv);
                    if constexpr (WP) st_at<float>(pb, e, pv);
                }
            }
        }
    }
    if constexpr (PHASE == DN_CG_DIRECTION || PHASE == PCG_DIRECTION) return;

    // workgroup sums -> workspace, arrival at the SAMPLE's counters; the sample's last arriver adds its G partials and updates its scalars
    // (the tails of the samples of a batch run side by side, each one memory round trip long)
    const int G = p.G;
    unsigned* counter = p.counter + (size_t)b * (DN_WS_HEADER / sizeof(unsigned));
    double* parts[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) parts[k] = p.part + ((size_t)k * p.batch + b) * G;
    double mine[NS];
    if constexpr (NS == 2) {
        block_sum2(s0, s1, red, tid, CG_THREADS);
        mine[0] = s0;
        mine[NS - 1] = s1;
    } else {
        mine[0] = block_sum(s0, red, tid, CG_THREADS);
    }
    if (tid == 0) {
        store_partials<NS, true>(parts, g, mine);
        flag = arrive_last<true>(counter, G, g) ? 1 : 0;
    }
    __syncthreads();
    if (!flag) return;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();

    // thread t adds partials t, t + 256, ... (eight requested ahead), then the fixed-order block sum: an order that depends on G alone
    double a[NS];
    sum_partials<NS, 8, true, true>(parts, G, tid, CG_THREADS, a);
    if constexpr (NS == 2) {
        block_sum2(a[0], a[NS - 1], red, tid, CG_THREADS);
    } else {
        a[0] = block_sum(a[0], red, tid, CG_THREADS);
    }
    if (tid != 0) return;
    CgState* s = stb;
    if constexpr (PHASE == DN_CG_INIT) {
        const double rr = a[NS - 1], at = (double)p.atol * (double)p.atol;
        s->rz = a[0];
        s->rr = rr;
        s->rr0 = rr;
        s->pq = 0.0;
        s->alpha = 0.f;
        s->beta = 0.f;
        s->active = rr > at ? 1 : 0;
        s->iterations = 0;
        s->flags = rr == rr ? 0 : DN_CG_BREAKDOWN;
    } else if constexpr (PHASE == DN_CG_DOT) {
        float al = 0.f;
        if (act) {
            const double pq = a[0];
            s->pq = pq;
            if (pq > 0.0) {
                al = (float)(s->rz / pq);
            } else {                                               // not SPD, or a NaN
                s->flags |= DN_CG_BREAKDOWN;
                s->active = 0;
            }
        }
        s->alpha = al;
    } else if constexpr (PHASE == PCG_RESID0) {
        const double rr = a[0], at = (double)p.atol * (double)p.atol;
        s->rz = 0.0;
        s->rr = rr;
        s->rr0 = rr;
        s->pq = 0.0;
        s->alpha = 0.f;
        s->beta = 0.f;
        s->active = rr > at ? 1 : 0;
        s->iterations = 0;
        s->flags = rr == rr ? 0 : DN_CG_BREAKDOWN;
    } else if constexpr (PHASE == PCG_UPDATE) {
        if (act) {
            const double rr = a[0];
            const double tt = (double)p.tol * (double)p.tol * s->rr0, at = (double)p.atol * (double)p.atol;
            s->rr = rr;
            s->iterations += 1;
            s->active = rr > (tt > at ? tt : at) ? 1 : 0;
            if (!(rr == rr)) s->flags |= DN_CG_BREAKDOWN;
        }
    } else if constexpr (PHASE == PCG_RZ) {
        if (act) {
            const double rzn = a[0], rz = s->rz;
            s->beta = rz > 0.0 ? (float)(rzn / rz) : 0.f;
            s->rz = rzn;
        }
    } else {
        if (act) {
            const double rzn = a[0], rr = a[NS - 1], rz = s->rz;
            const double tt = (double)p.tol * (double)p.tol * s->rr0, at = (double)p.atol * (double)p.atol;
            s->beta = rz > 0.0 ? (float)(rzn / rz) : 0.f;
            s->rz = rzn;
            s->rr = rr;
            s->iterations += 1;
            s->active = rr > (tt > at ? tt : at) ? 1 : 0;
            if (!(rr == rr)) s->flags |= DN_CG_BREAKDOWN;
        }
    }
    arrival_reset(counter);
}

}  // namespace dn

using namespace dn;

extern "C" int dn_poisson_diag(const dn_mesh* m, const dn_poisson_diag_args* a, void* stream) {
    if (!m) return DN_E_BADARG;
    if (m->nsd != 2 && m->nsd != 3) return DN_E_UNSUPPORTED;
    if (m->degree != 1 || m->ngp < 2 || m->ngp > 4) return DN_E_UNSUPPORTED;
    const int nz = m->nsd == 3 ? m->nz : 1;
    if (m->batch < 1 || m->batch > 65535 || m->nx < 2 || m->ny < 2 || (m->nsd == 3 && m->nz < 2)) return DN_E_BADARG;
    if ((int64_t)m->nx * m->ny * nz >= (1ll << 30) || nz > 65535) return DN_E_UNSUPPORTED;
    if (!a || !a->dinv) return DN_E_BADARG;
    if ((a->nu_batched | a->unit) & ~1) return DN_E_BADARG;

    DiagParams pp = {};
    for (int k = 0; k < 2; ++k) {
        const dn_dirichlet& d = a->bc[k];
        if (d.mask_kind == DN_MASK_BITS || d.mask_kind == DN_MASK_BOX) return DN_E_UNSUPPORTED;
        if (d.mask_kind != DN_MASK_F32 && d.mask_kind != DN_MASK_U8) return DN_E_BADARG;
        if (d.mask_batched & ~1) return DN_E_BADARG;
        pp.mask[k] = d.mask;
        pp.mask_kind[k] = !d.mask ? 0 : (d.mask_kind == DN_MASK_U8 ? 1 : 2);
        pp.mask_batched[k] = d.mask_batched;
    }
    pp.nu = a->nu;
    pp.nu_batched = a->nu_batched;
    pp.dinv = a->dinv;
    pp.wscale = a->wscale;
    pp.unit = a->unit;
    pp.nx = m->nx; pp.ny = m->ny; pp.nz = nz;
    for (int d = 0; d < m->nsd; ++d)
        for (int ia = 0; ia < 2; ++ia)
            for (int ib = 0; ib < 2; ++ib) {
                double mm = 0.0, dd = 0.0;
                for (int g = 0; g < m->ngp; ++g) {
                    const double na = m->basis[g][ia], nb = m->basis[g][ib], da = (double)m->dbasis[g][ia] * (double)m->scale[d];
                    mm += (double)m->gpw[g] * nb * na * na;
                    dd += (double)m->gpw[g] * nb * da * da;
                }
                pp.M[d][ia][ib] = (float)mm;
                pp.D[d][ia][ib] = (float)dd;
            }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 block(64), grid(((m->nx + 63) / 64) * m->ny, nz, m->batch);
    if (m->nsd == 2) hipLaunchKernelGGL(poisson_diag_kernel<2>, grid, block, 0, s, pp);
    else hipLaunchKernelGGL(poisson_diag_kernel<3>, grid, block, 0, s, pp);
    DN_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t dn_poisson_cg_workspace_bytes(int64_t n, int32_t batch) {
    if (n < 1 || n >= (1ll << 30) || batch < 1 || batch > 65535) return 0;
    int chunk, G;
    cg_geometry(n, chunk, G);
    return (DN_WS_HEADER + 2 * (int64_t)sizeof(double) * G) * batch;              // per sample: its counters, its partials
}

extern "C" int dn_poisson_cg(const dn_poisson_cg_args* a, void* stream) {
    if (!a) return DN_E_BADARG;
    if (a->phase < DN_CG_INIT || a->phase > DN_CG_DIRECTION) return DN_E_BADARG;
    if (a->n < 1 || a->batch < 1 || a->batch > 65535) return DN_E_BADARG;
    if (a->n >= (1ll << 30)) return DN_E_UNSUPPORTED;
    const int ph = a->phase;
    if (!a->state || !a->p) return DN_E_BADARG;
    if (ph != DN_CG_DIRECTION && !a->q) return DN_E_BADARG;
    if (ph != DN_CG_DOT && (!a->r || !a->dinv)) return DN_E_BADARG;
    if (ph == DN_CG_UPDATE && !a->x) return DN_E_BADARG;
    if (a->dinv_batched & ~1) return DN_E_BADARG;
    if (!(a->tol >= 0.f) || !(a->atol >= 0.f)) return DN_E_BADARG;
    // array bases are 16-byte aligned (a SAMPLE's base need not be); the state block 8
    for (const void* q : {(const void*)a->x, (const void*)a->r, (const void*)a->p, (const void*)a->q, (const void*)a->dinv})
        if (reinterpret_cast<uintptr_t>(q) & 15) return DN_E_BADARG;
    if (reinterpret_cast<uintptr_t>(a->state) & 7) return DN_E_BADARG;
    if (ph != DN_CG_DIRECTION) {
        if (!a->workspace || (reinterpret_cast<uintptr_t>(a->workspace) & 63)) return DN_E_BADARG;
        if (a->workspace_bytes < dn_poisson_cg_workspace_bytes(a->n, a->batch)) return DN_E_BADARG;
    }

    CgParams pp = {};
    pp.x = a->x; pp.r = a->r; pp.p = a->p; pp.q = a->q; pp.dinv = a->dinv;
    pp.dinv_batched = a->dinv_batched;
    pp.st = reinterpret_cast<CgState*>(a->state);
    pp.counter = reinterpret_cast<unsigned*>(a->workspace);
    pp.part = a->workspace ? reinterpret_cast<double*>(reinterpret_cast<char*>(a->workspace) + DN_WS_HEADER * a->batch) : nullptr;
    pp.n = (unsigned)a->n;
    cg_geometry(a->n, pp.chunk, pp.G);
    pp.batch = a->batch;
    pp.tol = a->tol; pp.atol = a->atol;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(pp.G, a->batch), block(CG_THREADS);
    switch (ph) {
        case DN_CG_INIT: hipLaunchKernelGGL(poisson_cg_kernel<DN_CG_INIT>, grid, block, 0, s, pp); break;
        case DN_CG_DOT: hipLaunchKernelGGL(poisson_cg_kernel<DN_CG_DOT>, grid, block, 0, s, pp); break;
        case DN_CG_UPDATE: hipLaunchKernelGGL(poisson_cg_kernel<DN_CG_UPDATE>, grid, block, 0, s, pp); break;
        default: hipLaunchKernelGGL(poisson_cg_kernel<DN_CG_DIRECTION>, grid, block, 0, s, pp); break;
    }
    DN_LAUNCH_CHECK();
    return 0;
}

extern "C" int dn_poisson_pcg(const dn_poisson_pcg_args* a, void* stream) {
    if (!a) return DN_E_BADARG;
    if (a->phase < DN_PCG_RESID0 || a->phase > DN_PCG_DIRECTION) return DN_E_BADARG;
    if (a->n < 1 || a->batch < 1 || a->batch > 65535) return DN_E_BADARG;
    if (a->n >= (1ll << 30)) return DN_E_UNSUPPORTED;
    const int ph = a->phase;
    if (!a->state) return DN_E_BADARG;
    if ((ph == DN_PCG_RESID0 || ph == DN_PCG_UPDATE) && (!a->r || !a->q)) return DN_E_BADARG;
    if (ph == DN_PCG_UPDATE && (!a->x || !a->p)) return DN_E_BADARG;
    if (ph == DN_PCG_RZ && (!a->r || !a->z)) return DN_E_BADARG;
    if (ph == DN_PCG_DIRECTION && (!a->p || !a->z)) return DN_E_BADARG;
    if (!(a->tol >= 0.f) || !(a->atol >= 0.f)) return DN_E_BADARG;
    for (const void* q : {(const void*)a->x, (const void*)a->r, (const void*)a->p, (const void*)a->q, (const void*)a->z})
        if (reinterpret_cast<uintptr_t>(q) & 15) return DN_E_BADARG;
    if (reinterpret_cast<uintptr_t>(a->state) & 7) return DN_E_BADARG;
    if (ph != DN_PCG_DIRECTION) {
        if (!a->workspace || (reinterpret_cast<uintptr_t>(a->workspace) & 63)) return DN_E_BADARG;
        if (a->workspace_bytes < dn_poisson_cg_workspace_bytes(a->n, a->batch)) return DN_E_BADARG;
    }

    CgParams pp = {};
    pp.x = a->x; pp.r = a->r; pp.p = a->p; pp.q = a->q; pp.z = a->z;
    pp.st = reinterpret_cast<CgState*>(a->state);
    pp.counter = reinterpret_cast<unsigned*>(a->workspace);
    pp.part = a->workspace ? reinterpret_cast<double*>(reinterpret_cast<char*>(a->workspace) + DN_WS_HEADER * a->batch) : nullptr;
    pp.n = (unsigned)a->n;
    cg_geometry(a->n, pp.chunk, pp.G);
    pp.batch = a->batch;
    pp.tol = a->tol; pp.atol = a->atol;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(pp.G, a->batch), block(CG_THREADS);
    switch (ph) {
        case DN_PCG_RESID0: hipLaunchKernelGGL(poisson_cg_kernel<PCG_RESID0>, grid, block, 0, s, pp); break;
        case DN_PCG_UPDATE: hipLaunchKernelGGL(poisson_cg_kernel<PCG_UPDATE>, grid, block, 0, s, pp); break;
        case DN_PCG_RZ: hipLaunchKernelGGL(poisson_cg_kernel<PCG_RZ>, grid, block, 0, s, pp); break;
        default: hipLaunchKernelGGL(poisson_cg_kernel<PCG_DIRECTION>, grid, block, 0, s, pp); break;
    }
    DN_LAUNCH_CHECK();
    return 0;
}
