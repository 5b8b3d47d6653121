// Fused 2-D strong-form least-squares loss on structured Q_P meshes and its gradient: dn_strongform_apply (include/diffnet_hip.h).
//
// The loss bodies of two scripts of the reference: examples/burgers/single_instance/01_2d_space_time.py:73-96 (Burgers.loss, space-time
// Burgers on Q2: u_t + u u_x with y as time) and examples/poisson/single_instance/10_manufactured_strong_form_higher_order.py:69-96
// (Poisson.loss, strong-form Poisson on Q3: u_xx + u_yy + f) -- the two Dirichlet substitutions, the Gauss-point evaluations including
// the second derivatives, the weighted sum of squares and, what autograd does for the scripts, its gradient with respect to u, in ONE
// launch that reads u once.
//
//   r_g    = ax u_x + ay u_y + b u u_x + dxx u_xx + dyy u_yy + fs f_g                     (of u~, u after the two conditions)
//   sum    = sum_{b,e,g} W_g r_g^2,   W_g = gpw_g wscale
//   grad_a = out_scale s sum_{e contains a} sum_g 2 W_g r_g ( ax Nx_a + ay Ny_a + b (N_a u_x + u Nx_a) + dxx Nxx_a + dyy Nyy_a )
//
// Same mapping as the element form of the FSDT kernel (fsdt.hip), with one field: a thread owns one element column of a strip and
// marches over element rows; the element is sum-factorised one x-Gauss point at a time (forward: u, u_x, u_y, u_xx, u_yy; transposed:
// the five flux coefficients 2 W r b u_x | 2 W r (ax + b u) | 2 W r ay | 2 W r dxx | 2 W r dyy on N | Nx | Ny | Nxx | Nyy); the
// contribution to the node column shared with the right neighbour goes through a double-buffered LDS slot; strip and chunk seams are
// closed by recomputing one layer / one column.  No atomics on the data path: every node is written once, by its owner, with the same
// additions in the same order under any launch plan and batch size.  The sum counts every element once (its owner thread, its own
// strip), per element in fp32, per thread in fp64, then the fixed-order fp64 reduction of dn_reduce.h.
//
// Optional inputs are compile-time forms: MASK (any condition), BCF (any value field), FK (forcing: constant / nodal / at the Gauss
// points), NL (b != 0), D2 (second-order terms present; never for P = 1, where they vanish identically).
#include <algorithm>
#include <cstdio>

#include "dn_reduce.h"

namespace dn {

struct SfParams {
    float b[4][4], dx[4][4], dy[4][4];     // 1-D tables at the Gauss points (derivatives scaled by 2/h)
    float dxx[4][4], dyy[4][4];            // second derivatives (scaled by (2/h)^2)
    float w2[4][4];                        // w[jg] * w[ig] * wscale
    float ax, ay, bb, cxx, cyy, fs, fconst, out_scale;
    const float* u;
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
    float* grad;
    double* part;                          // [nblocks] partial sums
    unsigned* counter;
    double* sum;
    int nx, ny, nelx, nely, rows_per_strip, want_sums;
};

// One element: nodal values F[jb][ib] (Fn: the nodal forcing); its contributions to the gradient are ADDED to g[jb][ib]; returns the
// element's sum_g W_g r_g^2.  fg: the forcing at the element's Gauss points (FK == 2).
template <int P, int NGP, int FK, bool NL, bool D2>
__device__ __forceinline__ float sf_elem(const SfParams& p, const float (&F)[P + 1][P + 1], const float (&Fn)[P + 1][P + 1],
                                         const float (&fg)[NGP * NGP], float (&g)[P + 1][P + 1]) {
    constexpr int NB = P + 1;
    float esum = 0.f;
#pragma unroll
    for (int ig = 0; ig < NGP; ++ig) {
        float tv[NB], td[NB], tdd[NB], tf[NB], rv[NB], rd[NB], rdd[NB];
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
            float a = 0.f, d = 0.f, dd = 0.f, ff = 0.f;
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) {
                a = fmaf(p.b[ig][ib], F[jb][ib], a);
                d = fmaf(p.dx[ig][ib], F[jb][ib], d);
                if constexpr (D2) dd = fmaf(p.dxx[ig][ib], F[jb][ib], dd);
                if constexpr (FK == 1) ff = fmaf(p.b[ig][ib], Fn[jb][ib], ff);
            }
            tv[jb] = a; td[jb] = d; tdd[jb] = dd; tf[jb] = ff;
            rv[jb] = 0.f; rd[jb] = 0.f; rdd[jb] = 0.f;
        }
#pragma unroll
        for (int jg = 0; jg < NGP; ++jg) {
            float v = 0.f, ux = 0.f, uy = 0.f, uxx = 0.f, uyy = 0.f, f = p.fconst;
            if constexpr (FK == 1) f = 0.f;
            if constexpr (FK == 2) f = fg[jg * NGP + ig];
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
                v = fmaf(p.b[jg][jb], tv[jb], v);
                ux = fmaf(p.b[jg][jb], td[jb], ux);
                uy = fmaf(p.dy[jg][jb], tv[jb], uy);
                if constexpr (D2) {
                    uxx = fmaf(p.b[jg][jb], tdd[jb], uxx);
                    uyy = fmaf(p.dyy[jg][jb], tv[jb], uyy);
                }
                if constexpr (FK == 1) f = fmaf(p.b[jg][jb], tf[jb], f);
            }
            float r = fmaf(p.ax, ux, fmaf(p.ay, uy, p.fs * f));
            if constexpr (NL) r = fmaf(p.bb * v, ux, r);
            if constexpr (D2) r = fmaf(p.cxx, uxx, fmaf(p.cyy, uyy, r));
            const float W = p.w2[jg][ig];
            const float Wr = W * r;
            esum = fmaf(Wr, r, esum);
            const float s = 2.f * Wr;
            float cx = s * p.ax;
            const float cy = s * p.ay;
            float cn = 0.f;
            if constexpr (NL) {
                cx = s * fmaf(p.bb, v, p.ax);
                cn = s * (p.bb * ux);
            }
            const float cxx = s * p.cxx, cyy = s * p.cyy;
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
                if constexpr (NL) rv[jb] = fmaf(p.b[jg][jb], cn, rv[jb]);
                rv[jb] = fmaf(p.dy[jg][jb], cy, rv[jb]);
                rd[jb] = fmaf(p.b[jg][jb], cx, rd[jb]);
                if constexpr (D2) {
                    rv[jb] = fmaf(p.dyy[jg][jb], cyy, rv[jb]);
                    rdd[jb] = fmaf(p.b[jg][jb], cxx, rdd[jb]);
                }
            }
        }
#pragma unroll
        for (int jb = 0; jb < NB; ++jb)
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) {
                g[jb][ib] = fmaf(p.b[ig][ib], rv[jb], g[jb][ib]);
                g[jb][ib] = fmaf(p.dx[ig][ib], rd[jb], g[jb][ib]);
                if constexpr (D2) g[jb][ib] = fmaf(p.dxx[ig][ib], rdd[jb], g[jb][ib]);
            }
    }
    return esum;
}

// grid = (chunks_x, strips_y, B), block = T threads; one element column per thread (chunks overlap by one thread column).  The P new node
// rows of layer k + 1 (and its Gauss-point forcing) are requested before the arithmetic of layer k; the finished rows of layer k are
// stored after that request (fsdt.hip has the reasons).
template <int P, int NGP, bool MASK, bool BCF, int FK, bool NL, bool D2>
__global__ void __launch_bounds__(256) strongform2d_kernel(const SfParams p) {
    constexpr int NB = P + 1;
    constexpr int NW = P;                  // nodes owned per thread per node row
    constexpr int G = NGP * NGP;
    static_assert(!(D2 && P == 1), "the second derivatives of a Q1 field vanish");
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
    const float okf = has_elem ? 1.f : 0.f;      // threads right of the mesh compute on clamped data, scaled by 0
    const unsigned exc = (unsigned)min(ex0, p.nelx - 1);

    const float* ub = p.u + (int64_t)b * nps;
    const float* fb = FK == 1 ? p.f + (p.f_batched ? (int64_t)b * nps : 0) : ub;
    const float* fgb = FK == 2 ? p.fgp + (p.f_batched ? (int64_t)b * G * nel : 0) : ub;
    float* ob = p.grad ? p.grad + (int64_t)b * nps : nullptr;
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

    __shared__ float xch[2][P][256];
    __shared__ double red[16];
    __shared__ int last_flag;

    float cu[NB][NB], fn[NB][NB], acc[NB][NB];
    unsigned fixed[NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) {
        fixed[r] = 0u;
#pragma unroll
        for (int n = 0; n < NB; ++n) { acc[r][n] = 0.f; fn[r][n] = 0.f; }
    }

    struct RawRow {
        float v[NW + 1], f[FK == 1 ? NW + 1 : 1];
        float mf[MASK ? 2 : 1][NW + 1], bf[BCF ? 2 : 1][NW + 1];
        uint8_t mb[MASK ? 2 : 1][NW + 1];
    };
    auto row_issue = [&](int yr, RawRow& w) {
        const unsigned rowoff = (unsigned)min(yr, ymax) * (unsigned)p.nx;
        load_seg<NW, false>(ub, rowoff, x0, p.nx, w.v);
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
    // landed row -> slot r: the two Dirichlet substitutions in order (condition 2 wins where both hold)
    auto row_consume = [&](const RawRow& w, int r) {
        unsigned bits = 0u;
#pragma unroll
        for (int n = 0; n <= NW; ++n) {
            float v = w.v[n];
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
            cu[r][n] = v;
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
    float pend[P][NW];
    unsigned pend_off[P];
    bool pend_st[P];
#pragma unroll
    for (int r = 0; r < P; ++r) pend_st[r] = false;
    auto flush_rows = [&]() {
#pragma unroll
        for (int r = 0; r < P; ++r) {
            if (pend_st[r]) store_seg<NW, false>(ob, pend_off[r], x0, p.nx, pend[r]);
            pend_st[r] = false;
        }
    };
    // Emit node row yr from acc[r] (+ the left neighbour's hand-over for n == 0); no gradient reaches a Dirichlet node
    auto emit_row = [&](int r, int slot, int yr, bool owned_row) {
        xch[par][r % P][tid] = acc[r][NW];
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS-only barrier (loads stay in flight)
        const float left = (tid > 0) ? xch[par][r % P][tid - 1] : 0.f;
#pragma unroll
        for (int n = 0; n < NW; ++n) {
            float v = (acc[r][n] + (n == 0 ? left : 0.f)) * gscale;
            v = (fixed[r] & (1u << n)) ? 0.f : v;
            pend[slot][n] = v;
        }
        pend_off[slot] = (unsigned)yr * (unsigned)p.nx;
        pend_st[slot] = owned_row && col_owner && ob != nullptr;
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
            {
                float g[NB][NB];
#pragma unroll
                for (int jb = 0; jb < NB; ++jb)
#pragma unroll
                    for (int ib = 0; ib < NB; ++ib) g[jb][ib] = 0.f;
                const float es = sf_elem<P, NGP, FK, NL, D2>(p, cu, fn, fgc, g);
                sq += (own_layer && col_owner && has_elem) ? (double)es : 0.0;
#pragma unroll
                for (int jb = 0; jb < NB; ++jb)
#pragma unroll
                    for (int ib = 0; ib < NB; ++ib) acc[jb][ib] = fmaf(okf, g[jb][ib], acc[jb][ib]);
            }
#pragma unroll
            for (int r = 0; r < P; ++r) emit_row(r, r, ey * P + r, own_layer);
            par ^= 1;
#pragma unroll
            for (int n = 0; n <= NW; ++n) {
                cu[0][n] = cu[P][n];
                fn[0][n] = fn[P][n];
                acc[0][n] = acc[P][n];
#pragma unroll
                for (int r = 1; r <= P; ++r) acc[r][n] = 0.f;
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

#ifndef SF_DEGREE      // the host side of the entry points: strongform.hip alone
static inline int sf_ceil_div(int a, int b) { return (a + b - 1) / b; }

struct SfGeom { int T, chunks, R, strips; };

constexpr int SF_MIN_ROWS = 4;             // shortest strip the library chooses (element rows): a strip recomputes one layer

// Threads per workgroup by utilisation of the last chunk (wider wins at equal utilisation), then the strip height: enough waves for ~4
// per SIMD at the price of one recomputed layer per strip -- the rule of the FSDT element form, whose element this one resembles.
// "PLAN_FSDT" ("T,R") overrides both, as it does there; the results do not depend on the plan.
static SfGeom sf_plan(const dn_mesh* m) {
    SfGeom g;
    const int P = m->degree;
    const int Q = (m->nx - 1) / P + 1;          // logical thread columns (one per element + the closing column)
    const int nely = (m->ny - 1) / P;
    double best = -1.0;
    g.T = 64; g.chunks = 1;
    for (int T = 64; T <= 256; T += 64) {
        const int chunks = Q <= T ? 1 : sf_ceil_div(Q - 1, T - 1);
        const double score = (double)Q / ((double)chunks * T) + 0.0003 * T;
        if (score > best) { best = score; g.T = T; g.chunks = chunks; }
    }
    const long long per_strip = (long long)g.chunks * m->batch * (g.T / 64);
    int R = 32;
    while (R > SF_MIN_ROWS && per_strip * sf_ceil_div(nely, R) < 4096) R /= 2;
    const char* e = config(CFG_PLAN_FSDT);
    int T, RR;
    if (e && sscanf(e, "%d,%d", &T, &RR) == 2 && T >= 64 && T <= 256 && T % 64 == 0 && RR >= 1) {
        g.T = T; R = RR;
        g.chunks = Q <= T ? 1 : sf_ceil_div(Q - 1, T - 1);
    }
    g.R = std::max(1, std::min(R, nely));
    g.strips = sf_ceil_div(nely, g.R);
    return g;
}

static int sf_validate(const dn_mesh* m) {
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
static inline int64_t sf_workspace_bytes(const dn_mesh* m) {
    const int P = m->degree;
    const int Q = (m->nx - 1) / P + 1, nely = (m->ny - 1) / P;
    const int64_t chunks = Q <= 64 ? 1 : sf_ceil_div(Q - 1, 63);
    return DN_WS_HEADER + (int64_t)sizeof(double) * chunks * nely * m->batch;
}

#endif

#define SF_LAUNCH(...) hipLaunchKernelGGL((strongform2d_kernel<__VA_ARGS__>), grid, block, 0, s, pp)

// sel: 0 no condition, 1 conditions with constants, 2 with a value field
template <int P, int NGP, int FK, bool NL, bool D2>
static void sf_launch_mask(const SfParams& pp, int sel, dim3 grid, dim3 block, hipStream_t s) {
    if (sel == 2) SF_LAUNCH(P, NGP, true, true, FK, NL, D2);
    else if (sel == 1) SF_LAUNCH(P, NGP, true, false, FK, NL, D2);
    else SF_LAUNCH(P, NGP, false, false, FK, NL, D2);
}

template <int P, int NGP, bool NL, bool D2>
static void sf_launch_fk(const SfParams& pp, int sel, dim3 grid, dim3 block, hipStream_t s) {
    if (pp.fgp) sf_launch_mask<P, NGP, 2, NL, D2>(pp, sel, grid, block, s);
    else if (pp.f) sf_launch_mask<P, NGP, 1, NL, D2>(pp, sel, grid, block, s);
    else sf_launch_mask<P, NGP, 0, NL, D2>(pp, sel, grid, block, s);
}

template <int P, int NGP>
void sf_launch_terms(const SfParams& pp, int sel, bool nl, bool d2, dim3 grid, dim3 block, hipStream_t s) {
    if constexpr (P > 1) {
        if (d2) {
            if (nl) sf_launch_fk<P, NGP, true, true>(pp, sel, grid, block, s);
            else sf_launch_fk<P, NGP, false, true>(pp, sel, grid, block, s);
            return;
        }
    }
    if (nl) sf_launch_fk<P, NGP, true, false>(pp, sel, grid, block, s);
    else sf_launch_fk<P, NGP, false, false>(pp, sel, grid, block, s);
}

#ifndef SF_DEGREE
// The Q2 and Q3 instantiations compile in translation units of their own (strongform_q2.hip, strongform_q3.hip)
extern template void sf_launch_terms<2, 3>(const SfParams&, int, bool, bool, dim3, dim3, hipStream_t);
extern template void sf_launch_terms<2, 4>(const SfParams&, int, bool, bool, dim3, dim3, hipStream_t);
extern template void sf_launch_terms<3, 3>(const SfParams&, int, bool, bool, dim3, dim3, hipStream_t);
extern template void sf_launch_terms<3, 4>(const SfParams&, int, bool, bool, dim3, dim3, hipStream_t);
#else
template void sf_launch_terms<SF_DEGREE, 3>(const SfParams&, int, bool, bool, dim3, dim3, hipStream_t);
template void sf_launch_terms<SF_DEGREE, 4>(const SfParams&, int, bool, bool, dim3, dim3, hipStream_t);
#endif

}  // namespace dn

#ifndef SF_DEGREE
using namespace dn;

extern "C" int64_t dn_strongform_workspace_bytes(const dn_mesh* m) {
    if (sf_validate(m) != 0) return DN_E_BADARG;
    return sf_workspace_bytes(m);
}

extern "C" int dn_strongform_apply(const dn_mesh* m, const dn_strongform_args* a, void* stream) {
    int rc = sf_validate(m);
    if (rc) return rc;
    if (!a || !a->u) return DN_E_BADARG;
    if (!a->grad && !a->sum) return DN_E_BADARG;
    if (a->f && a->f_gp) return DN_E_BADARG;
    if (a->f_batched & ~1) return DN_E_BADARG;
    for (int k = 0; k < 2; ++k) {
        const dn_dirichlet& d = a->bc[k];
        if (d.mask_kind == DN_MASK_BITS || d.mask_kind == DN_MASK_BOX) return DN_E_UNSUPPORTED;     // expand them: dn_unpack_mask_bits
        if (d.mask_kind != DN_MASK_F32 && d.mask_kind != DN_MASK_U8) return DN_E_BADARG;
        if ((d.mask_batched | d.field_batched) & ~1) return DN_E_BADARG;
        if (d.field && !d.mask) return DN_E_BADARG;                           // a value field without its mask
    }
    if (a->sum && (!a->workspace || a->workspace_bytes < sf_workspace_bytes(m))) return DN_E_WORKSPACE;
    const SfGeom g = sf_plan(m);

    SfParams pp;
    const double sx = m->scale[0], sy = m->scale[1];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const bool in = i < m->ngp && j <= m->degree;
            pp.b[i][j] = in ? m->basis[i][j] : 0.f;
            pp.dx[i][j] = in ? (float)(m->dbasis[i][j] * sx) : 0.f;
            pp.dy[i][j] = in ? (float)(m->dbasis[i][j] * sy) : 0.f;
            pp.dxx[i][j] = in ? (float)(a->d2basis[i][j] * sx * sx) : 0.f;
            pp.dyy[i][j] = in ? (float)(a->d2basis[i][j] * sy * sy) : 0.f;
            pp.w2[i][j] = (i < m->ngp && j < m->ngp) ? m->gpw[i] * (m->gpw[j] * a->wscale) : 0.f;
        }
    pp.ax = a->ax; pp.ay = a->ay; pp.bb = a->b; pp.cxx = a->dxx; pp.cyy = a->dyy; pp.fs = a->fs;
    pp.fconst = (a->f || a->f_gp) ? 0.f : a->f_value;
    pp.out_scale = a->out_scale;
    pp.u = a->u; pp.f = a->f; pp.fgp = a->f_gp; pp.f_batched = a->f_batched;
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
    pp.grad = a->grad;
    pp.counter = reinterpret_cast<unsigned*>(a->workspace);
    pp.part = a->workspace ? reinterpret_cast<double*>(reinterpret_cast<char*>(a->workspace) + DN_WS_HEADER) : nullptr;
    pp.sum = a->sum;
    pp.nx = m->nx; pp.ny = m->ny;
    pp.nelx = (m->nx - 1) / m->degree; pp.nely = (m->ny - 1) / m->degree;
    pp.rows_per_strip = g.R;
    pp.want_sums = a->sum ? 1 : 0;

    const dim3 grid(g.chunks, g.strips, m->batch), block(g.T);
    const int sel = mask ? (bcf ? 2 : 1) : 0;
    const bool nl = a->b != 0.f;
    const bool d2 = m->degree > 1 && (a->dxx != 0.f || a->dyy != 0.f);       // Q1: identically zero, no work spent on them
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (m->degree * 10 + m->ngp) {
        case 12: sf_launch_terms<1, 2>(pp, sel, nl, d2, grid, block, s); break;
        case 13: sf_launch_terms<1, 3>(pp, sel, nl, d2, grid, block, s); break;
        case 14: sf_launch_terms<1, 4>(pp, sel, nl, d2, grid, block, s); break;
        case 23: sf_launch_terms<2, 3>(pp, sel, nl, d2, grid, block, s); break;
        case 24: sf_launch_terms<2, 4>(pp, sel, nl, d2, grid, block, s); break;
        case 33: sf_launch_terms<3, 3>(pp, sel, nl, d2, grid, block, s); break;
        default: sf_launch_terms<3, 4>(pp, sel, nl, d2, grid, block, s); break;
    }
    DN_LAUNCH_CHECK();
    return 0;
}
#endif
