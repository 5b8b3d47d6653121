// Fused 2-D Helmholtz energy and weak-form residual on structured Q_P meshes: dn_helmholtz_apply (include/diffnet_hip.h).
//
// The loss body the two Helmholtz scripts of the reference share, examples/poisson/single_instance/14_helmholtz_mms.py:37-63 and
// 14_helmholtz_ddelta.py:37-63 (Poisson.loss: the Poisson energy plus a reaction term -khh^2 u^2 / 2) -- the two Dirichlet substitutions,
// five Gauss-point evaluations, the weighted sum and, what autograd does for the scripts, its gradient with respect to u -- in ONE launch
// that reads u once; with alpha = gamma = beta = 1 the same launch is the assembled weak-form residual and its sum of squares.
//
//   energy = sum_{b,e,g} W_g ( c nu_g |grad u~_g|^2 - cr sg_g u~_g^2 - fs u~_g f_g ),   W_g = gpw_g wscale
//   out_a  = out_scale zero_on_dirichlet( sum_{e contains a} sum_g W_g ( alpha nu_g gradN_a . grad u~_g - gamma sg_g N_a u~_g - beta N_a f_g ) )
//   sumsq  = sum over (b, nodes) of (out / out_scale)^2
//
// Same mapping as the strong-form kernel (strongform.hip; the element form of fsdt.hip has the reasons): a thread owns one element column
// of a strip and marches over element rows; the element is sum-factorised one x-Gauss point at a time (forward: u, u_x, u_y and, where
// they are fields, nu, sigma and f; transposed: the three flux coefficients -W (gamma sg u + beta f) | W alpha nu u_x | W alpha nu u_y on
// N | Nx | Ny); the contribution to the node column shared with the right neighbour goes through a double-buffered LDS slot; strip and
// chunk seams are closed by recomputing one layer / one column.  No atomics on the data path: every node is written once, by its owner,
// with the same additions in the same order under any launch plan and batch size.  The energy counts every element once (its owner
// thread, its own strip) and sumsq every node once (its owner, after its value is complete): per element / node row in fp32, per thread
// in fp64, then the fixed-order fp64 reduction of dn_reduce.h.
//
// Optional inputs are compile-time forms: MASK (any condition), BCF (any value field), FK (forcing: constant / nodal / at the Gauss
// points), CF (coefficients: 0 nu = 1 and no reaction term, 1 nu = 1 and a constant sigma, 2 nu and / or sigma a nodal field -- the one
// that is not a field is its constant there).  27 forms per (degree, rule).
#include <algorithm>
#include <cstdio>

#include "dn_reduce.h"

namespace dn {

struct HhParams {
    float b[4][4], dx[4][4], dy[4][4];     // 1-D tables at the Gauss points (derivatives scaled by 2/h)
    float w2[4][4];                        // w[jg] * w[ig] * wscale
    float c, cr, fs, alpha, gamma, beta, sgconst, fconst, out_scale;
    const float* u;
    const float* nu;                       // CF == 2: nodal coefficient or nullptr (1)
    const float* sg;                       // CF == 2: nodal sigma or nullptr (sgconst)
    int nu_batched, sg_batched;
    const float* f;                        // FK == 1: nodal forcing
    const float* fgp;                      // FK == 2: (B | 1, G, nely, nelx)
    int f_batched;
    const void* mask[2];
    int mask_kind[2];                      // 0: none, 1: uint8 (!= 0), 2: fp32 (> 0.5)
    int mask_batched[2];
    const float* bcf[2];
    int bcf_batched[2];
    float bcv[2];
    float* out;
    double* part;                          // [2][nblocks] partial sums: energy, sumsq
    unsigned* counter;
    double* energy;
    double* sumsq;
    int nx, ny, nelx, nely, rows_per_strip, want_sums;
};

// One element: nodal values F[jb][ib] of u~ (Kn, Sn, Fn: nodal nu, sigma, forcing); its contributions to out are ADDED to g[jb][ib];
// returns the element's energy sum_g W_g (...).  fg: the forcing at the element's Gauss points (FK == 2).
template <int P, int NGP, int FK, int CF>
__device__ __forceinline__ float hh_elem(const HhParams& p, const float (&F)[P + 1][P + 1], const float (&Kn)[P + 1][P + 1],
                                         const float (&Sn)[P + 1][P + 1], const float (&Fn)[P + 1][P + 1], const float (&fg)[NGP * NGP],
                                         float (&g)[P + 1][P + 1]) {
    constexpr int NB = P + 1;
    float esum = 0.f;
#pragma unroll
    for (int ig = 0; ig < NGP; ++ig) {
        float tv[NB], td[NB], tk[NB], ts[NB], tf[NB], rv[NB], rd[NB];
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
            float a = 0.f, d = 0.f, kk = 0.f, ss = 0.f, ff = 0.f;
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) {
                a = fmaf(p.b[ig][ib], F[jb][ib], a);
                d = fmaf(p.dx[ig][ib], F[jb][ib], d);
                if constexpr (CF == 2) {
                    kk = fmaf(p.b[ig][ib], Kn[jb][ib], kk);
                    ss = fmaf(p.b[ig][ib], Sn[jb][ib], ss);
                }
                if constexpr (FK == 1) ff = fmaf(p.b[ig][ib], Fn[jb][ib], ff);
            }
            tv[jb] = a; td[jb] = d; tk[jb] = kk; ts[jb] = ss; tf[jb] = ff;
            rv[jb] = 0.f; rd[jb] = 0.f;
        }
#pragma unroll
        for (int jg = 0; jg < NGP; ++jg) {
            float v = 0.f, ux = 0.f, uy = 0.f, nug = 1.f, sgg = p.sgconst, f = p.fconst;
            if constexpr (CF == 2) { nug = 0.f; sgg = 0.f; }
            if constexpr (FK == 1) f = 0.f;
            if constexpr (FK == 2) f = fg[jg * NGP + ig];
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
                v = fmaf(p.b[jg][jb], tv[jb], v);
                ux = fmaf(p.b[jg][jb], td[jb], ux);
                uy = fmaf(p.dy[jg][jb], tv[jb], uy);
                if constexpr (CF == 2) {
                    nug = fmaf(p.b[jg][jb], tk[jb], nug);
                    sgg = fmaf(p.b[jg][jb], ts[jb], sgg);
                }
                if constexpr (FK == 1) f = fmaf(p.b[jg][jb], tf[jb], f);
            }
            const float W = p.w2[jg][ig];
            const float Wk = W * nug;
            float e = (p.c * Wk) * fmaf(ux, ux, uy * uy);
            e = fmaf(-(p.fs * W) * v, f, e);
            float cn = -(p.beta * W) * f;
            if constexpr (CF != 0) {
                const float Wsv = (W * sgg) * v;
                e = fmaf(-p.cr * Wsv, v, e);
                cn = fmaf(-p.gamma, Wsv, cn);
            }
            esum += e;
            const float ak = p.alpha * Wk;
            const float cx = ak * ux, cy = ak * uy;
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
                rv[jb] = fmaf(p.b[jg][jb], cn, rv[jb]);
                rv[jb] = fmaf(p.dy[jg][jb], cy, rv[jb]);
                rd[jb] = fmaf(p.b[jg][jb], cx, rd[jb]);
            }
        }
#pragma unroll
        for (int jb = 0; jb < NB; ++jb)
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) {
                g[jb][ib] = fmaf(p.b[ig][ib], rv[jb], g[jb][ib]);
                g[jb][ib] = fmaf(p.dx[ig][ib], rd[jb], g[jb][ib]);
            }
    }
    return esum;
}

// grid = (chunks_x, strips_y, B), block = T threads; one element column per thread (chunks overlap by one thread column).  The P new node
// rows of layer k + 1 (and its Gauss-point forcing) are requested before the arithmetic of layer k; the finished rows of layer k are
// stored after that request (fsdt.hip has the reasons).
template <int P, int NGP, bool MASK, bool BCF, int FK, int CF>
__global__ void __launch_bounds__(256) helmholtz2d_kernel(const HhParams p) {
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
    const float okf = has_elem ? 1.f : 0.f;      // threads right of the mesh compute on clamped data, scaled by 0
    const unsigned exc = (unsigned)min(ex0, p.nelx - 1);

    const float* ub = p.u + (int64_t)b * nps;
    const float* kb = (CF == 2 && p.nu) ? p.nu + (p.nu_batched ? (int64_t)b * nps : 0) : ub;
    const float* sb = (CF == 2 && p.sg) ? p.sg + (p.sg_batched ? (int64_t)b * nps : 0) : ub;
    const float* fb = FK == 1 ? p.f + (p.f_batched ? (int64_t)b * nps : 0) : ub;
    const float* fgb = FK == 2 ? p.fgp + (p.f_batched ? (int64_t)b * G * nel : 0) : ub;
    float* ob = p.out ? p.out + (int64_t)b * nps : nullptr;
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
    const float oscale = p.out_scale;

    __shared__ float xch[2][P][256];
    __shared__ double red[16];
    __shared__ int last_flag;

    float cu[NB][NB], kn[NB][NB], sn[NB][NB], fn[NB][NB], acc[NB][NB];
    unsigned fixed[NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) {
        fixed[r] = 0u;
#pragma unroll
        for (int n = 0; n < NB; ++n) { acc[r][n] = 0.f; fn[r][n] = 0.f; kn[r][n] = 1.f; sn[r][n] = p.sgconst; }
    }

    struct RawRow {
        float v[NW + 1], f[FK == 1 ? NW + 1 : 1];
        float k[CF == 2 ? NW + 1 : 1], s[CF == 2 ? NW + 1 : 1];
        float mf[MASK ? 2 : 1][NW + 1], bf[BCF ? 2 : 1][NW + 1];
        uint8_t mb[MASK ? 2 : 1][NW + 1];
    };
    auto row_issue = [&](int yr, RawRow& w) {
        const unsigned rowoff = (unsigned)min(yr, ymax) * (unsigned)p.nx;
        load_seg<NW, false>(ub, rowoff, x0, p.nx, w.v);
        if constexpr (FK == 1) load_seg<NW, false>(fb, rowoff, x0, p.nx, w.f);
        if constexpr (CF == 2) {
            if (p.nu) load_seg<NW, false>(kb, rowoff, x0, p.nx, w.k);
            if (p.sg) load_seg<NW, false>(sb, rowoff, x0, p.nx, w.s);
        }
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
            if constexpr (CF == 2) {
                kn[r][n] = p.nu ? w.k[n] : 1.f;
                sn[r][n] = p.sg ? w.s[n] : p.sgconst;
            }
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

    double en = 0.0, ssq = 0.0;
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
    // Emit node row yr from acc[r] (+ the left neighbour's hand-over for n == 0): the row is complete here, so its owner adds its
    // squares to sumsq; nothing reaches a Dirichlet node
    auto emit_row = [&](int r, int slot, int yr, bool owned_row) {
        xch[par][r % P][tid] = acc[r][NW];
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS-only barrier (loads stay in flight)
        const float left = (tid > 0) ? xch[par][r % P][tid - 1] : 0.f;
        const bool mine = owned_row && col_owner;
        float rs = 0.f;
#pragma unroll
        for (int n = 0; n < NW; ++n) {
            float v = acc[r][n] + (n == 0 ? left : 0.f);
            v = (fixed[r] & (1u << n)) ? 0.f : v;
            rs = (x0 + n < p.nx) ? fmaf(v, v, rs) : rs;
            pend[slot][n] = v * oscale;
        }
        ssq += mine ? (double)rs : 0.0;
        pend_off[slot] = (unsigned)yr * (unsigned)p.nx;
        pend_st[slot] = mine && ob != nullptr;
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
                const float es = hh_elem<P, NGP, FK, CF>(p, cu, kn, sn, fn, fgc, g);
                en += (own_layer && col_owner && has_elem) ? (double)es : 0.0;
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
                kn[0][n] = kn[P][n];
                sn[0][n] = sn[P][n];
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
        const int nblocks = launch_workgroups();
        double* const parts[2] = {p.part, p.part + nblocks};
        block_sum2(en, ssq, red, tid, nthreads);
        const double mine[2] = {en, ssq};
        double tot[2];
        if (last_arriver_sums<2, 8, false, true>(parts, p.counter, mine, tid, nthreads, &last_flag, tot)) {
            block_sum2(tot[0], tot[1], red, tid, nthreads);
            if (tid == 0) {
                if (p.energy) p.energy[0] = tot[0];
                if (p.sumsq) p.sumsq[0] = tot[1];
                arrival_reset(p.counter);
                p.counter[DN_WS_TICKET_WORD] = 0u;
            }
        }
    }
}

#ifndef HH_DEGREE      // the host side of the entry points: helmholtz.hip alone
static inline int hh_ceil_div(int a, int b) { return (a + b - 1) / b; }

struct HhGeom { int T, chunks, R, strips; };

constexpr int HH_MIN_ROWS = 4;             // shortest strip the library chooses (element rows): a strip recomputes one layer

// The plan of the strong-form kernel, whose element this one resembles: threads per workgroup by utilisation of the last chunk (wider
// wins at equal utilisation), then the strip height: enough waves for ~4 per SIMD at the price of one recomputed layer per strip.
// "PLAN_FSDT" ("T,R") overrides both, as it does there; out does not depend on the plan.
static HhGeom hh_plan(const dn_mesh* m) {
    HhGeom g;
    const int P = m->degree;
    const int Q = (m->nx - 1) / P + 1;          // logical thread columns (one per element + the closing column)
    const int nely = (m->ny - 1) / P;
    double best = -1.0;
    g.T = 64; g.chunks = 1;
    for (int T = 64; T <= 256; T += 64) {
        const int chunks = Q <= T ? 1 : hh_ceil_div(Q - 1, T - 1);
        const double score = (double)Q / ((double)chunks * T) + 0.0003 * T;
        if (score > best) { best = score; g.T = T; g.chunks = chunks; }
    }
    const long long per_strip = (long long)g.chunks * m->batch * (g.T / 64);
    int R = 32;
    while (R > HH_MIN_ROWS && per_strip * hh_ceil_div(nely, R) < 4096) R /= 2;
    const char* e = config(CFG_PLAN_FSDT);
    int T, RR;
    if (e && sscanf(e, "%d,%d", &T, &RR) == 2 && T >= 64 && T <= 256 && T % 64 == 0 && RR >= 1) {
        g.T = T; R = RR;
        g.chunks = Q <= T ? 1 : hh_ceil_div(Q - 1, T - 1);
    }
    g.R = std::max(1, std::min(R, nely));
    g.strips = hh_ceil_div(nely, g.R);
    return g;
}

static int hh_validate(const dn_mesh* m) {
    if (!m || m->nsd != 2) return DN_E_BADARG;
    if (m->degree < 1 || m->degree > 3 || m->ngp < 2 || m->ngp > 4 || (m->degree > 1 && m->ngp < 3)) return DN_E_UNSUPPORTED;
    if (m->batch < 1 || m->batch > 65535 || m->nx < 2 || m->ny < 2) return DN_E_BADARG;
    if ((m->nx - 1) % m->degree || (m->ny - 1) % m->degree) return DN_E_BADARG;
    if ((int64_t)m->nx * m->ny >= (1ll << 30)) return DN_E_UNSUPPORTED;
    const int64_t nel = (int64_t)((m->nx - 1) / m->degree) * ((m->ny - 1) / m->degree);
    if (nel * m->ngp * m->ngp >= (1ll << 30) || (m->ny - 1) / m->degree > 65535) return DN_E_UNSUPPORTED;     // 32-bit offsets; grid.y
    return 0;
}

// Two partial sums per workgroup, for an upper bound of the workgroups over every launch plan (one-wave chunks, one-row strips): the
// size does not change with "PLAN_FSDT"
static inline int64_t hh_workspace_bytes(const dn_mesh* m) {
    const int P = m->degree;
    const int Q = (m->nx - 1) / P + 1, nely = (m->ny - 1) / P;
    const int64_t chunks = Q <= 64 ? 1 : hh_ceil_div(Q - 1, 63);
    return DN_WS_HEADER + 2 * (int64_t)sizeof(double) * chunks * nely * m->batch;
}

#endif

#define HH_LAUNCH(...) hipLaunchKernelGGL((helmholtz2d_kernel<__VA_ARGS__>), grid, block, 0, s, pp)

// sel: 0 no condition, 1 conditions with constants, 2 with a value field
template <int P, int NGP, int FK, int CF>
static void hh_launch_mask(const HhParams& pp, int sel, dim3 grid, dim3 block, hipStream_t s) {
    if (sel == 2) HH_LAUNCH(P, NGP, true, true, FK, CF);
    else if (sel == 1) HH_LAUNCH(P, NGP, true, false, FK, CF);
    else HH_LAUNCH(P, NGP, false, false, FK, CF);
}

template <int P, int NGP, int CF>
static void hh_launch_fk(const HhParams& pp, int sel, dim3 grid, dim3 block, hipStream_t s) {
    if (pp.fgp) hh_launch_mask<P, NGP, 2, CF>(pp, sel, grid, block, s);
    else if (pp.f) hh_launch_mask<P, NGP, 1, CF>(pp, sel, grid, block, s);
    else hh_launch_mask<P, NGP, 0, CF>(pp, sel, grid, block, s);
}

// cf: 0 nu = 1 and no reaction term, 1 nu = 1 and a constant sigma, 2 a nodal nu and / or sigma
template <int P, int NGP>
void hh_launch_coef(const HhParams& pp, int sel, int cf, dim3 grid, dim3 block, hipStream_t s) {
    if (cf == 2) hh_launch_fk<P, NGP, 2>(pp, sel, grid, block, s);
    else if (cf == 1) hh_launch_fk<P, NGP, 1>(pp, sel, grid, block, s);
    else hh_launch_fk<P, NGP, 0>(pp, sel, grid, block, s);
}

#ifndef HH_DEGREE
// The Q2 and Q3 instantiations compile in translation units of their own (helmholtz_q2.hip, helmholtz_q3.hip)
extern template void hh_launch_coef<2, 3>(const HhParams&, int, int, dim3, dim3, hipStream_t);
extern template void hh_launch_coef<2, 4>(const HhParams&, int, int, dim3, dim3, hipStream_t);
extern template void hh_launch_coef<3, 3>(const HhParams&, int, int, dim3, dim3, hipStream_t);
extern template void hh_launch_coef<3, 4>(const HhParams&, int, int, dim3, dim3, hipStream_t);
#else
template void hh_launch_coef<HH_DEGREE, 3>(const HhParams&, int, int, dim3, dim3, hipStream_t);
template void hh_launch_coef<HH_DEGREE, 4>(const HhParams&, int, int, dim3, dim3, hipStream_t);
#endif

}  // namespace dn

#ifndef HH_DEGREE
using namespace dn;

extern "C" int64_t dn_helmholtz_workspace_bytes(const dn_mesh* m) {
    if (hh_validate(m) != 0) return DN_E_BADARG;
    return hh_workspace_bytes(m);
}

extern "C" int dn_helmholtz_apply(const dn_mesh* m, const dn_helmholtz_args* a, void* stream) {
    int rc = hh_validate(m);
    if (rc) return rc;
    if (!a || !a->u) return DN_E_BADARG;
    if (!a->out && !a->energy && !a->sumsq) return DN_E_BADARG;
    if (a->f && a->f_gp) return DN_E_BADARG;
    if ((a->f_batched | a->nu_batched | a->sigma_batched) & ~1) return DN_E_BADARG;
    for (int k = 0; k < 2; ++k) {
        const dn_dirichlet& d = a->bc[k];
        if (d.mask_kind == DN_MASK_BITS || d.mask_kind == DN_MASK_BOX) return DN_E_UNSUPPORTED;     // expand them: dn_unpack_mask_bits
        if (d.mask_kind != DN_MASK_F32 && d.mask_kind != DN_MASK_U8) return DN_E_BADARG;
        if ((d.mask_batched | d.field_batched) & ~1) return DN_E_BADARG;
        if (d.field && !d.mask) return DN_E_BADARG;                           // a value field without its mask
    }
    const bool sums = a->energy || a->sumsq;
    if (sums && (!a->workspace || a->workspace_bytes < hh_workspace_bytes(m))) return DN_E_WORKSPACE;
    const HhGeom g = hh_plan(m);

    HhParams pp;
    const double sx = m->scale[0], sy = m->scale[1];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const bool in = i < m->ngp && j <= m->degree;
            pp.b[i][j] = in ? m->basis[i][j] : 0.f;
            pp.dx[i][j] = in ? (float)(m->dbasis[i][j] * sx) : 0.f;
            pp.dy[i][j] = in ? (float)(m->dbasis[i][j] * sy) : 0.f;
            pp.w2[i][j] = (i < m->ngp && j < m->ngp) ? m->gpw[i] * (m->gpw[j] * a->wscale) : 0.f;
        }
    pp.c = a->c; pp.cr = a->cr; pp.fs = a->fs; pp.alpha = a->alpha; pp.gamma = a->gamma; pp.beta = a->beta;
    pp.sgconst = a->sigma ? 0.f : a->sigma_value;
    pp.fconst = (a->f || a->f_gp) ? 0.f : a->f_value;
    pp.out_scale = a->out_scale;
    pp.u = a->u; pp.nu = a->nu; pp.sg = a->sigma; pp.nu_batched = a->nu_batched; pp.sg_batched = a->sigma_batched;
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
    pp.out = a->out;
    pp.counter = reinterpret_cast<unsigned*>(a->workspace);
    pp.part = a->workspace ? reinterpret_cast<double*>(reinterpret_cast<char*>(a->workspace) + DN_WS_HEADER) : nullptr;
    pp.energy = a->energy;
    pp.sumsq = a->sumsq;
    pp.nx = m->nx; pp.ny = m->ny;
    pp.nelx = (m->nx - 1) / m->degree; pp.nely = (m->ny - 1) / m->degree;
    pp.rows_per_strip = g.R;
    pp.want_sums = sums ? 1 : 0;

    const dim3 grid(g.chunks, g.strips, m->batch), block(g.T);
    const int sel = mask ? (bcf ? 2 : 1) : 0;
    const int cf = (a->nu || a->sigma) ? 2 : (a->sigma_value != 0.f ? 1 : 0);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (m->degree * 10 + m->ngp) {
        case 12: hh_launch_coef<1, 2>(pp, sel, cf, grid, block, s); break;
        case 13: hh_launch_coef<1, 3>(pp, sel, cf, grid, block, s); break;
        case 14: hh_launch_coef<1, 4>(pp, sel, cf, grid, block, s); break;
        case 23: hh_launch_coef<2, 3>(pp, sel, cf, grid, block, s); break;
        case 24: hh_launch_coef<2, 4>(pp, sel, cf, grid, block, s); break;
        case 33: hh_launch_coef<3, 3>(pp, sel, cf, grid, block, s); break;
        default: hh_launch_coef<3, 4>(pp, sel, cf, grid, block, s); break;
    }
    DN_LAUNCH_CHECK();
    return 0;
}
#endif
