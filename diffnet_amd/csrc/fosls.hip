// Fused 2-D first-order-system least-squares loss on structured Q_P meshes and its three gradients: dn_fosls_apply (include/diffnet_hip.h).
//
// The loss body of examples/poisson/single_instance/11_manufactured_strong_form_two_dofs.py:37-71 of the reference (Poisson.loss on the
// three nodal fields u, mx, my: the flux m = nu grad u and its divergence as a first-order system) -- the two Dirichlet substitutions of
// u, the eleven Gauss-point evaluations, the weighted sums of squares and, what autograd does for the script, the gradients with respect
// to u, mx and my, in ONE launch that reads every field once.
//
//   qx = mx - nu u_x,  qy = my - nu u_y,  d = mx_x + my_y + fs f                          (of u~, u after the two conditions)
//   sum     = sum_{b,e,g} W_g ( wq (qx^2 + qy^2) + wd d^2 ),   W_g = gpw_g wscale
//   gu_a    = out_scale s sum -2 W wq nu (qx Nx_a + qy Ny_a)                              (zero on the Dirichlet nodes)
//   gmx_a   = out_scale s sum  2 W (wq qx N_a + wd d Nx_a)
//   gmy_a   = out_scale s sum  2 W (wq qy N_a + wd d Ny_a)
//
// The mapping of strongform.hip with three fields and first derivatives only: a thread owns one element column of a strip and marches
// over element rows; the element is sum-factorised one x-Gauss point at a time (forward: u_x, u_y, mx, mx_x, my, my_y, nu, f;
// transposed: the coefficients -nu cqx | -nu cqy on Nx | Ny of u, cqx | cd on N | Nx of mx, cqy | cd on N | Ny of my, with
// cq = 2 W wq q, cd = 2 W wd d), added straight into the three node accumulators; the contributions to the node column shared with the
// right neighbour go through a double-buffered LDS slot (one barrier per node row for the three fields); strip and chunk seams are
// closed by recomputing one layer / one column.  No atomics on the data path: every node of every gradient is written once, by its
// owner, with the same additions in the same order under any launch plan and batch size.  The sum counts every element once, per
// element in fp32, per thread in fp64, then the fixed-order fp64 reduction of dn_reduce.h.
//
// The three fields (and the three gradients) are addressed by one pointer each plus one element stride between samples, so the packed
// (B, 3, ny, nx) parameter of the script is read, and its packed gradient written, in place.
//
// Optional inputs are compile-time forms: MASK (any condition), BCF (any value field), FK (forcing: constant / nodal / at the Gauss
// points), NUF (nu: constant / nodal field).
#include <algorithm>
#include <cstdio>

#include "dn_reduce.h"

namespace dn {

struct FoParams {
    float b[4][4], dx[4][4], dy[4][4];     // 1-D tables at the Gauss points (derivatives scaled by 2/h)
    float w2[4][4];                        // w[jg] * w[ig] * wscale
    float wq, wd, fs, fconst, nuconst, out_scale;
    const float* fld[3];                   // u, mx, my
    int64_t fld_stride, grad_stride;       // elements between samples
    const float* nu;                       // NUF: nodal coefficient
    int nu_batched;
    const float* f;                        // FK == 1: nodal forcing
    const float* fgp;                      // FK == 2: (B | 1, G, nely, nelx)
    int f_batched;
    const void* mask[2];
    int mask_kind[2];                      // 0: none, 1: uint8 (!= 0), 2: fp32 (> 0.5)
    int mask_batched[2];
    const float* bcf[2];
    int bcf_batched[2];
    float bcv[2];
    const float* in_scale;
    float* grad[3];
    double* part;                          // [nblocks] partial sums
    unsigned* counter;
    double* sum;
    int nx, ny, nelx, nely, rows_per_strip, want_sums;
};

// One element: nodal values F[k][jb][ib] of u~, mx, my (Cn: the nodal coefficient, Fn: the nodal forcing); its contributions to the
// three gradients, times `ok`, are ADDED to g[k][jb][ib]; returns the element's sum_g W_g (wq |q|^2 + wd d^2) times `ok`.
// fg: the forcing at the element's Gauss points (FK == 2).
template <int P, int NGP, int FK, bool NUF>
__device__ __forceinline__ float fo_elem(const FoParams& p, const float (&F)[3][P + 1][P + 1], const float (&Cn)[P + 1][P + 1],
                                         const float (&Fn)[P + 1][P + 1], const float (&fg)[NGP * NGP], float ok,
                                         float (&g)[3][P + 1][P + 1]) {
    constexpr int NB = P + 1;
    float esum = 0.f;
#pragma unroll
    for (int ig = 0; ig < NGP; ++ig) {
        // x stage: values (v) and x-derivatives (d) of the node rows at this x-Gauss point
        float uv[NB], ud[NB], av[NB], ad[NB], bv[NB], tn[NB], tf[NB];
        float ruv[NB], rud[NB], rav[NB], rad[NB], rbv[NB];
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
            float u0 = 0.f, u1 = 0.f, a0 = 0.f, a1 = 0.f, b0 = 0.f, nn = 0.f, ff = 0.f;
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) {
                u0 = fmaf(p.b[ig][ib], F[0][jb][ib], u0);
                u1 = fmaf(p.dx[ig][ib], F[0][jb][ib], u1);
                a0 = fmaf(p.b[ig][ib], F[1][jb][ib], a0);
                a1 = fmaf(p.dx[ig][ib], F[1][jb][ib], a1);
                b0 = fmaf(p.b[ig][ib], F[2][jb][ib], b0);
                if constexpr (NUF) nn = fmaf(p.b[ig][ib], Cn[jb][ib], nn);
                if constexpr (FK == 1) ff = fmaf(p.b[ig][ib], Fn[jb][ib], ff);
            }
            uv[jb] = u0; ud[jb] = u1; av[jb] = a0; ad[jb] = a1; bv[jb] = b0; tn[jb] = nn; tf[jb] = ff;
            ruv[jb] = 0.f; rud[jb] = 0.f; rav[jb] = 0.f; rad[jb] = 0.f; rbv[jb] = 0.f;
        }
#pragma unroll
        for (int jg = 0; jg < NGP; ++jg) {
            float ux = 0.f, uy = 0.f, mx = 0.f, mxx = 0.f, my = 0.f, myy = 0.f, nu = p.nuconst, f = p.fconst;
            if constexpr (NUF) nu = 0.f;
            if constexpr (FK == 1) f = 0.f;
            if constexpr (FK == 2) f = fg[jg * NGP + ig];
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
                ux = fmaf(p.b[jg][jb], ud[jb], ux);
                uy = fmaf(p.dy[jg][jb], uv[jb], uy);
                mx = fmaf(p.b[jg][jb], av[jb], mx);
                mxx = fmaf(p.b[jg][jb], ad[jb], mxx);
                my = fmaf(p.b[jg][jb], bv[jb], my);
                myy = fmaf(p.dy[jg][jb], bv[jb], myy);
                if constexpr (NUF) nu = fmaf(p.b[jg][jb], tn[jb], nu);
                if constexpr (FK == 1) f = fmaf(p.b[jg][jb], tf[jb], f);
            }
            const float qx = fmaf(-nu, ux, mx), qy = fmaf(-nu, uy, my);
            const float d = fmaf(p.fs, f, mxx + myy);
            const float W = p.w2[jg][ig] * ok;
            const float Wq = W * p.wq, Wd = W * p.wd;
            esum = fmaf(Wq, fmaf(qx, qx, qy * qy), esum);
            esum = fmaf(Wd * d, d, esum);
            const float cqx = 2.f * Wq * qx, cqy = 2.f * Wq * qy, cd = 2.f * Wd * d;
            const float cux = -nu * cqx, cuy = -nu * cqy;
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
                rud[jb] = fmaf(p.b[jg][jb], cux, rud[jb]);
                ruv[jb] = fmaf(p.dy[jg][jb], cuy, ruv[jb]);
                rav[jb] = fmaf(p.b[jg][jb], cqx, rav[jb]);
                rad[jb] = fmaf(p.b[jg][jb], cd, rad[jb]);
                rbv[jb] = fmaf(p.b[jg][jb], cqy, rbv[jb]);
                rbv[jb] = fmaf(p.dy[jg][jb], cd, rbv[jb]);
            }
        }
#pragma unroll
        for (int jb = 0; jb < NB; ++jb)
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) {
                g[0][jb][ib] = fmaf(p.b[ig][ib], ruv[jb], g[0][jb][ib]);
                g[0][jb][ib] = fmaf(p.dx[ig][ib], rud[jb], g[0][jb][ib]);
                g[1][jb][ib] = fmaf(p.b[ig][ib], rav[jb], g[1][jb][ib]);
                g[1][jb][ib] = fmaf(p.dx[ig][ib], rad[jb], g[1][jb][ib]);
                g[2][jb][ib] = fmaf(p.b[ig][ib], rbv[jb], g[2][jb][ib]);
            }
    }
    return esum;
}

// grid = (chunks_x, strips_y, B), block = T threads; one element column per thread (chunks overlap by one thread column).  The P new node
// rows of layer k + 1 (and its Gauss-point forcing) are requested before the arithmetic of layer k; the finished rows of layer k are
// stored after that request (fsdt.hip has the reasons).
template <int P, int NGP, bool MASK, bool BCF, int FK, bool NUF>
__global__ void __launch_bounds__(256) fosls2d_kernel(const FoParams p) {
    constexpr int NB = P + 1;
    constexpr int NW = P;                  // nodes owned per thread per node row
    constexpr int G = NGP * NGP;
    static_assert(MASK || !BCF, "a value field belongs to a condition");
    const int T = (int)blockDim.x, tid = (int)threadIdx.x;
    const int chunk = blockIdx.x, b = blockIdx.z;
    const int R = p.rows_per_strip;
    const int ey_own = (int)blockIdx.y * R;
    const int q = chunk * (T - 1) + tid;
    const int ex0 = q, x0 = ex0 * P;
    const bool col_owner = !(chunk > 0 && tid == 0);
    const int64_t nps = (int64_t)p.nx * p.ny;
    const int nel = p.nelx * p.nely;
    const int ey_begin = ey_own > 0 ? ey_own - 1 : ey_own;        // the layer under the strip's first node row is recomputed
    const int ey_end = min(ey_own + R, p.nely);
    const int ymax = p.ny - 1;
    const bool has_elem = ex0 < p.nelx;
    const float okf = has_elem ? 1.f : 0.f;      // threads right of the mesh compute on clamped data, weighted by 0
    const unsigned exc = (unsigned)min(ex0, p.nelx - 1);

    const float* fldb[3];
    float* ob[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        fldb[k] = p.fld[k] + (int64_t)b * p.fld_stride;
        ob[k] = p.grad[k] ? p.grad[k] + (int64_t)b * p.grad_stride : nullptr;
    }
    const float* ub = fldb[0];
    const float* nub = NUF ? p.nu + (p.nu_batched ? (int64_t)b * nps : 0) : ub;
    const float* fb = FK == 1 ? p.f + (p.f_batched ? (int64_t)b * nps : 0) : ub;
    const float* fgb = FK == 2 ? p.fgp + (p.f_batched ? (int64_t)b * G * nel : 0) : ub;
    const float* bcfb[2];
    const float* mfp[2];
    const uint8_t* mbp[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        bcfb[k] = p.bcf[k] ? p.bcf[k] + (p.bcf_batched[k] ? (int64_t)b * nps : 0) : ub;
        const int64_t mo = p.mask_batched[k] ? (int64_t)b * nps : 0;
        mfp[k] = p.mask_kind[k] == 2 ? reinterpret_cast<const float*>(p.mask[k]) + mo : ub;
        mbp[k] = p.mask_kind[k] == 1 ? reinterpret_cast<const uint8_t*>(p.mask[k]) + mo : reinterpret_cast<const uint8_t*>(ub);
    }
    float gscale = p.out_scale;
    if (p.in_scale) gscale *= p.in_scale[0];

    __shared__ float xch[2][P][3][256];
    __shared__ double red[16];
    __shared__ int last_flag;

    float cu[3][NB][NB], cn[NB][NB], fn[NB][NB], acc[3][NB][NB];
    unsigned fixed[NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) {
        fixed[r] = 0u;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            cn[r][n] = 0.f; fn[r][n] = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k][r][n] = 0.f;
        }
    }

    struct RawRow {
        float v[3][NW + 1], c[NUF ? NW + 1 : 1], f[FK == 1 ? NW + 1 : 1];
        float mf[MASK ? 2 : 1][NW + 1], bf[BCF ? 2 : 1][NW + 1];
        uint8_t mb[MASK ? 2 : 1][NW + 1];
    };
    auto row_issue = [&](int yr, RawRow& w) {
        const unsigned rowoff = (unsigned)min(yr, ymax) * (unsigned)p.nx;
#pragma unroll
        for (int k = 0; k < 3; ++k) load_seg<NW, false>(fldb[k], rowoff, x0, p.nx, w.v[k]);
        if constexpr (NUF) load_seg<NW, false>(nub, rowoff, x0, p.nx, w.c);
        if constexpr (FK == 1) load_seg<NW, false>(fb, rowoff, x0, p.nx, w.f);
        if constexpr (MASK) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (p.mask_kind[k] == 2) load_seg<NW, false>(mfp[k], rowoff, x0, p.nx, w.mf[k]);
                else if (p.mask_kind[k] == 1) load_seg<NW, false>(mbp[k], rowoff, x0, p.nx, w.mb[k]);
            }
        }
        if constexpr (BCF) {
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (p.bcf[k]) load_seg<NW, false>(bcfb[k], rowoff, x0, p.nx, w.bf[k]);
        }
    };
    // landed row -> slot r: the two Dirichlet substitutions of u in order (condition 2 wins where both hold); mx and my are free
    auto row_consume = [&](const RawRow& w, int r) {
        unsigned bits = 0u;
#pragma unroll
        for (int n = 0; n <= NW; ++n) {
            float v = w.v[0][n];
            if constexpr (MASK) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const bool fx = p.mask_kind[k] == 2 ? (w.mf[k][n] > 0.5f) : (p.mask_kind[k] == 1 ? (w.mb[k][n] != 0) : false);
                    float bv = p.bcv[k];
                    if constexpr (BCF) bv = p.bcf[k] ? w.bf[k][n] : bv;
                    v = fx ? bv : v;
                    bits |= fx ? (1u << n) : 0u;
                }
            }
            cu[0][r][n] = v;
            cu[1][r][n] = w.v[1][n];
            cu[2][r][n] = w.v[2][n];
            if constexpr (NUF) cn[r][n] = w.c[n];
            if constexpr (FK == 1) fn[r][n] = w.f[n];
        }
        fixed[r] = bits;
    };
    auto fg_issue = [&](int ey, float (&w)[G]) {
        if constexpr (FK == 2) {
            const unsigned eoff = (unsigned)min(ey, p.nely - 1) * (unsigned)p.nelx + exc;
#pragma unroll
            for (int gq = 0; gq < G; ++gq) w[gq] = ld_at<float>(fgb, eoff + (unsigned)(gq * nel));
        }
    };

    double sq = 0.0;
    int par = 0;

    // finished node rows wait here until flush_rows() stores them
    float pend[P][3][NW];
    unsigned pend_off[P];
    bool pend_st[P];
#pragma unroll
    for (int r = 0; r < P; ++r) pend_st[r] = false;
    auto flush_rows = [&]() {
#pragma unroll
        for (int r = 0; r < P; ++r) {
            if (pend_st[r]) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (ob[k]) store_seg<NW, false>(ob[k], pend_off[r], x0, p.nx, pend[r][k]);
            }
            pend_st[r] = false;
        }
    };
    // Emit node row yr from acc[.][r] (+ the left neighbour's hand-over for n == 0); no gradient of u reaches a Dirichlet node
    auto emit_row = [&](int r, int slot, int yr, bool owned_row) {
#pragma unroll
        for (int k = 0; k < 3; ++k) xch[par][r % P][k][tid] = acc[k][r][NW];
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS-only barrier (loads stay in flight)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float left = (tid > 0) ? xch[par][r % P][k][tid - 1] : 0.f;
#pragma unroll
            for (int n = 0; n < NW; ++n) {
                float v = (acc[k][r][n] + (n == 0 ? left : 0.f)) * gscale;
                if (k == 0) v = (fixed[r] & (1u << n)) ? 0.f : v;
                pend[slot][k][n] = v;
            }
        }
        pend_off[slot] = (unsigned)yr * (unsigned)p.nx;
        pend_st[slot] = owned_row && col_owner;
    };

    {
        RawRow W[P];
        float fgw[FK == 2 ? G : 1], fgc[G];
#pragma unroll
        for (int gq = 0; gq < G; ++gq) fgc[gq] = 0.f;
        {
            RawRow w0;
            row_issue(ey_begin * P, w0);
#pragma unroll
            for (int r = 1; r <= P; ++r) row_issue(ey_begin * P + r, W[r - 1]);       // all P + 1 rows of the first layer in flight together
            if constexpr (FK == 2) fg_issue(ey_begin, fgw);
            row_consume(w0, 0);
        }
        for (int ey = ey_begin; ey < ey_end; ++ey) {
#pragma unroll
            for (int r = 1; r <= P; ++r) row_consume(W[r - 1], r);
            if constexpr (FK == 2) {
#pragma unroll
                for (int gq = 0; gq < G; ++gq) fgc[gq] = fgw[gq];
            }
#pragma unroll
            for (int r = 1; r <= P; ++r) row_issue((ey + 1) * P + r, W[r - 1]);      // rows beyond the mesh re-read the last one (unused)
            if constexpr (FK == 2) fg_issue(ey + 1, fgw);
            flush_rows();
            const bool own_layer = ey >= ey_own;
            const float es = fo_elem<P, NGP, FK, NUF>(p, cu, cn, fn, fgc, okf, acc);
            sq += (own_layer && col_owner && has_elem) ? (double)es : 0.0;
#pragma unroll
            for (int r = 0; r < P; ++r) emit_row(r, r, ey * P + r, own_layer);
            par ^= 1;
#pragma unroll
            for (int n = 0; n <= NW; ++n) {
                cn[0][n] = cn[P][n];
                fn[0][n] = fn[P][n];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    cu[k][0][n] = cu[k][P][n];
                    acc[k][0][n] = acc[k][P][n];
#pragma unroll
                    for (int r = 1; r <= P; ++r) acc[k][r][n] = 0.f;
                }
            }
            fixed[0] = fixed[P];
        }
        flush_rows();
        if (ey_end == p.nely) {
            emit_row(0, 0, p.ny - 1, true);
            flush_rows();
        }
    }

    if (p.want_sums) {
        const int nthreads = (int)blockDim.x;
        double* const parts[1] = {p.part};
        const double mine[1] = {block_sum(sq, red, tid, nthreads)};
        double tot[1];
        if (last_arriver_sums<1, 8, false, true>(parts, p.counter, mine, tid, nthreads, &last_flag, tot)) {
            const double e = block_sum(tot[0], red, tid, nthreads);
            if (tid == 0) {
                p.sum[0] = e;
                arrival_reset(p.counter);
                p.counter[DN_WS_TICKET_WORD] = 0u;
            }
        }
    }
}

#ifndef FO_DEGREE      // the host side of the entry points: fosls.hip alone
static inline int fo_ceil_div(int a, int b) { return (a + b - 1) / b; }

struct FoGeom { int T, chunks, R, strips; };

constexpr int FO_MIN_ROWS = 4;             // shortest strip the library chooses (element rows): a strip recomputes one layer

// The plan of the strong-form kernel (strongform.hip: threads per workgroup by utilisation of the last chunk, then the strip height for
// ~4 waves per SIMD at the price of one recomputed layer per strip).  "PLAN_FSDT" ("T,R") overrides both, as it does there; the
// results do not depend on the plan.
static FoGeom fo_plan(const dn_mesh* m) {
    FoGeom g;
    const int P = m->degree;
    const int Q = (m->nx - 1) / P + 1;          // logical thread columns (one per element + the closing column)
    const int nely = (m->ny - 1) / P;
    double best = -1.0;
    g.T = 64; g.chunks = 1;
    for (int T = 64; T <= 256; T += 64) {
        const int chunks = Q <= T ? 1 : fo_ceil_div(Q - 1, T - 1);
        const double score = (double)Q / ((double)chunks * T) + 0.0003 * T;
        if (score > best) { best = score; g.T = T; g.chunks = chunks; }
    }
    const long long per_strip = (long long)g.chunks * m->batch * (g.T / 64);
    int R = 32;
    while (R > FO_MIN_ROWS && per_strip * fo_ceil_div(nely, R) < 4096) R /= 2;
    const char* e = config(CFG_PLAN_FSDT);
    int T, RR;
    if (e && sscanf(e, "%d,%d", &T, &RR) == 2 && T >= 64 && T <= 256 && T % 64 == 0 && RR >= 1) {
        g.T = T; R = RR;
        g.chunks = Q <= T ? 1 : fo_ceil_div(Q - 1, T - 1);
    }
    g.R = std::max(1, std::min(R, nely));
    g.strips = fo_ceil_div(nely, g.R);
    return g;
}

static int fo_validate(const dn_mesh* m) {
    if (!m || m->nsd != 2) return DN_E_BADARG;
    if (m->degree < 1 || m->degree > 3 || m->ngp < 2 || m->ngp > 4 || (m->degree > 1 && m->ngp < 3)) return DN_E_UNSUPPORTED;
    if (m->batch < 1 || m->batch > 65535 || m->nx < 2 || m->ny < 2) return DN_E_BADARG;
    if ((m->nx - 1) % m->degree || (m->ny - 1) % m->degree) return DN_E_BADARG;
    if ((int64_t)m->nx * m->ny >= (1ll << 30)) return DN_E_UNSUPPORTED;
    const int64_t nel = (int64_t)((m->nx - 1) / m->degree) * ((m->ny - 1) / m->degree);
    if (nel * m->ngp * m->ngp >= (1ll << 30) || (m->ny - 1) / m->degree > 65535) return DN_E_UNSUPPORTED;     // 32-bit offsets; grid.y
    return 0;
}

// An upper bound over every launch plan (one-wave chunks, one-row strips): the size does not change with "PLAN_FSDT"
static inline int64_t fo_workspace_bytes(const dn_mesh* m) {
    const int P = m->degree;
    const int Q = (m->nx - 1) / P + 1, nely = (m->ny - 1) / P;
    const int64_t chunks = Q <= 64 ? 1 : fo_ceil_div(Q - 1, 63);
    return DN_WS_HEADER + (int64_t)sizeof(double) * chunks * nely * m->batch;
}

#endif

#define FO_LAUNCH(...) hipLaunchKernelGGL((fosls2d_kernel<__VA_ARGS__>), grid, block, 0, s, pp)

// sel: 0 no condition, 1 conditions with constants, 2 with a value field
template <int P, int NGP, int FK, bool NUF>
static void fo_launch_mask(const FoParams& pp, int sel, dim3 grid, dim3 block, hipStream_t s) {
    if (sel == 2) FO_LAUNCH(P, NGP, true, true, FK, NUF);
    else if (sel == 1) FO_LAUNCH(P, NGP, true, false, FK, NUF);
    else FO_LAUNCH(P, NGP, false, false, FK, NUF);
}

template <int P, int NGP, bool NUF>
static void fo_launch_fk(const FoParams& pp, int sel, dim3 grid, dim3 block, hipStream_t s) {
    if (pp.fgp) fo_launch_mask<P, NGP, 2, NUF>(pp, sel, grid, block, s);
    else if (pp.f) fo_launch_mask<P, NGP, 1, NUF>(pp, sel, grid, block, s);
    else fo_launch_mask<P, NGP, 0, NUF>(pp, sel, grid, block, s);
}

template <int P, int NGP>
void fo_launch_forms(const FoParams& pp, int sel, dim3 grid, dim3 block, hipStream_t s) {
    if (pp.nu) fo_launch_fk<P, NGP, true>(pp, sel, grid, block, s);
    else fo_launch_fk<P, NGP, false>(pp, sel, grid, block, s);
}

#ifndef FO_DEGREE
// The Q2 and Q3 instantiations compile in translation units of their own (fosls_q2.hip, fosls_q3.hip)
extern template void fo_launch_forms<2, 3>(const FoParams&, int, dim3, dim3, hipStream_t);
extern template void fo_launch_forms<2, 4>(const FoParams&, int, dim3, dim3, hipStream_t);
extern template void fo_launch_forms<3, 3>(const FoParams&, int, dim3, dim3, hipStream_t);
extern template void fo_launch_forms<3, 4>(const FoParams&, int, dim3, dim3, hipStream_t);
#else
template void fo_launch_forms<FO_DEGREE, 3>(const FoParams&, int, dim3, dim3, hipStream_t);
template void fo_launch_forms<FO_DEGREE, 4>(const FoParams&, int, dim3, dim3, hipStream_t);
#endif

}  // namespace dn

#ifndef FO_DEGREE
using namespace dn;

extern "C" int64_t dn_fosls_workspace_bytes(const dn_mesh* m) {
    if (fo_validate(m) != 0) return DN_E_BADARG;
    return fo_workspace_bytes(m);
}

extern "C" int dn_fosls_apply(const dn_mesh* m, const dn_fosls_args* a, void* stream) {
    int rc = fo_validate(m);
    if (rc) return rc;
    if (!a || !a->u || !a->mx || !a->my) return DN_E_BADARG;
    const bool any_grad = a->grad_u || a->grad_mx || a->grad_my;
    if (!any_grad && !a->sum) return DN_E_BADARG;
    const int64_t nps = (int64_t)m->nx * m->ny;
    if (a->field_stride < nps || (any_grad && a->grad_stride < nps)) return DN_E_BADARG;
    if (a->f && a->f_gp) return DN_E_BADARG;
    if ((a->f_batched | a->nu_batched) & ~1) return DN_E_BADARG;
    for (int k = 0; k < 2; ++k) {
        const dn_dirichlet& d = a->bc[k];
        if (d.mask_kind == DN_MASK_BITS || d.mask_kind == DN_MASK_BOX) return DN_E_UNSUPPORTED;     // expand them: dn_unpack_mask_bits
        if (d.mask_kind != DN_MASK_F32 && d.mask_kind != DN_MASK_U8) return DN_E_BADARG;
        if ((d.mask_batched | d.field_batched) & ~1) return DN_E_BADARG;
        if (d.field && !d.mask) return DN_E_BADARG;                           // a value field without its mask
    }
    if (a->sum && (!a->workspace || a->workspace_bytes < fo_workspace_bytes(m))) return DN_E_WORKSPACE;
    const FoGeom g = fo_plan(m);

    FoParams pp;
    const double sx = m->scale[0], sy = m->scale[1];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const bool in = i < m->ngp && j <= m->degree;
            pp.b[i][j] = in ? m->basis[i][j] : 0.f;
            pp.dx[i][j] = in ? (float)(m->dbasis[i][j] * sx) : 0.f;
            pp.dy[i][j] = in ? (float)(m->dbasis[i][j] * sy) : 0.f;
            pp.w2[i][j] = (i < m->ngp && j < m->ngp) ? m->gpw[i] * (m->gpw[j] * a->wscale) : 0.f;
        }
    pp.wq = a->wq; pp.wd = a->wd; pp.fs = a->fs;
    pp.fconst = (a->f || a->f_gp) ? 0.f : a->f_value;
    pp.nuconst = a->nu ? 0.f : a->nu_value;
    pp.out_scale = a->out_scale;
    pp.fld[0] = a->u; pp.fld[1] = a->mx; pp.fld[2] = a->my;
    pp.fld_stride = a->field_stride; pp.grad_stride = any_grad ? a->grad_stride : 0;
    pp.nu = a->nu; pp.nu_batched = a->nu_batched;
    pp.f = a->f; pp.fgp = a->f_gp; pp.f_batched = a->f_batched;
    bool mask = false, bcf = false;
    for (int k = 0; k < 2; ++k) {
        const dn_dirichlet& d = a->bc[k];
        pp.mask[k] = d.mask;
        pp.mask_kind[k] = !d.mask ? 0 : (d.mask_kind == DN_MASK_U8 ? 1 : 2);
        pp.mask_batched[k] = d.mask_batched;
        pp.bcf[k] = d.field;
        pp.bcf_batched[k] = d.field_batched;
        pp.bcv[k] = d.value;
        mask = mask || d.mask;
        bcf = bcf || d.field;
    }
    pp.in_scale = a->in_scale;
    pp.grad[0] = a->grad_u; pp.grad[1] = a->grad_mx; pp.grad[2] = a->grad_my;
    pp.counter = reinterpret_cast<unsigned*>(a->workspace);
    pp.part = a->workspace ? reinterpret_cast<double*>(reinterpret_cast<char*>(a->workspace) + DN_WS_HEADER) : nullptr;
    pp.sum = a->sum;
    pp.nx = m->nx; pp.ny = m->ny;
    pp.nelx = (m->nx - 1) / m->degree; pp.nely = (m->ny - 1) / m->degree;
    pp.rows_per_strip = g.R;
    pp.want_sums = a->sum ? 1 : 0;

    const dim3 grid(g.chunks, g.strips, m->batch), block(g.T);
    const int sel = mask ? (bcf ? 2 : 1) : 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (m->degree * 10 + m->ngp) {
        case 12: fo_launch_forms<1, 2>(pp, sel, grid, block, s); break;
        case 13: fo_launch_forms<1, 3>(pp, sel, grid, block, s); break;
        case 14: fo_launch_forms<1, 4>(pp, sel, grid, block, s); break;
        case 23: fo_launch_forms<2, 3>(pp, sel, grid, block, s); break;
        case 24: fo_launch_forms<2, 4>(pp, sel, grid, block, s); break;
        case 33: fo_launch_forms<3, 3>(pp, sel, grid, block, s); break;
        default: fo_launch_forms<3, 4>(pp, sel, grid, block, s); break;
    }
    DN_LAUNCH_CHECK();
    return 0;
}
#endif
