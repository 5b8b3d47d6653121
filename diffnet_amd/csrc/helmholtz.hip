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
#include "elem2d_common.h"      // everything the kernel shares with strongform.hip and fosls.hip: parameters, the march, plan, checks, launch switch

namespace dn {

struct HhParams : Elem2dParams {
    float c, cr, fs, alpha, gamma, beta, sgconst, fconst, out_scale;
    const float* u;
    const float* nu;                       // CF == 2: nodal coefficient or nullptr (1)
    const float* sg;                       // CF == 2: nodal sigma or nullptr (sgconst)
    int nu_batched, sg_batched;
    float* out;
    double* energy;                        // sum 0: every element once
    double* sumsq;                         // sum 1: every node once (its owner, after its value is complete)
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

// What the march (elem2d_march.inl) asks of the operator: one field, two sums (energy, sumsq)
template <int P_, int NGP_, int FK_, int CF>
struct HhOp {
    static constexpr int P = P_, NGP = NGP_, FK = FK_, NF = 1, NS = 2, NB = P + 1;
    static constexpr bool FOLDS_OK = false;
    struct Raw { float v[NB], k[CF == 2 ? NB : 1], s[CF == 2 ? NB : 1]; };
    const float* ub;
    const float* kb;
    const float* sb;
    float oscale;
    float cu[NB][NB], kn[NB][NB], sn[NB][NB];

    __device__ __forceinline__ void init(const HhParams& p, int b, int64_t nps) {
        ub = p.u + (int64_t)b * nps;
        kb = (CF == 2 && p.nu) ? p.nu + (p.nu_batched ? (int64_t)b * nps : 0) : ub;
        sb = (CF == 2 && p.sg) ? p.sg + (p.sg_batched ? (int64_t)b * nps : 0) : ub;
    }
    __device__ __forceinline__ void start(const HhParams& p) {
        oscale = p.out_scale;
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int n = 0; n < NB; ++n) { kn[r][n] = 1.f; sn[r][n] = p.sgconst; }
    }
    __device__ __forceinline__ float* out_base(const HhParams& p, int, int b, int64_t nps) const { return p.out ? p.out + (int64_t)b * nps : nullptr; }
    template <class F>
    __device__ __forceinline__ void issue(const HhParams& p, unsigned rowoff, int x0, Raw& w, F issue_f) const {
        load_seg<P, false>(ub, rowoff, x0, p.nx, w.v);
        issue_f();
        if constexpr (CF == 2) {
            if (p.nu) load_seg<P, false>(kb, rowoff, x0, p.nx, w.k);
            if (p.sg) load_seg<P, false>(sb, rowoff, x0, p.nx, w.s);
        }
    }
    __device__ __forceinline__ float raw_u(const Raw& w, int n) const { return w.v[n]; }
    __device__ __forceinline__ void put(const HhParams& p, const Raw& w, int r, int n, float v) {
        cu[r][n] = v;
        if constexpr (CF == 2) {
            kn[r][n] = p.nu ? w.k[n] : 1.f;
            sn[r][n] = p.sg ? w.s[n] : p.sgconst;
        }
    }
    __device__ __forceinline__ void shift(int n) {
        cu[0][n] = cu[P][n];
        kn[0][n] = kn[P][n];
        sn[0][n] = sn[P][n];
    }
    __device__ __forceinline__ float element(const HhParams& p, const float (&fn)[NB][NB], const float (&fg)[NGP * NGP], float,
                                             float (&g)[1][NB][NB]) const {
        return hh_elem<P, NGP, FK, CF>(p, cu, kn, sn, fn, fg, g[0]);
    }
    // nothing reaches a Dirichlet node; the row's squares (before out_scale) go to sumsq
    __device__ __forceinline__ float finish_row(const HhParams& p, int, float (&row)[P], unsigned fixed, int x0) const {
        float rs = 0.f;
#pragma unroll
        for (int n = 0; n < P; ++n) {
            const float v = (fixed & (1u << n)) ? 0.f : row[n];
            rs = (x0 + n < p.nx) ? fmaf(v, v, rs) : rs;
            row[n] = v * oscale;
        }
        return rs;
    }
    __device__ __forceinline__ void write_sums(const HhParams& p, const double (&tot)[2]) const {
        if (p.energy) p.energy[0] = tot[0];
        if (p.sumsq) p.sumsq[0] = tot[1];
    }
};

template <int P, int NGP, bool MASK, bool BCF, int FK, int CF>
__global__ void __launch_bounds__(256) helmholtz2d_kernel(const HhParams p) {
    using Op = HhOp<P, NGP, FK, CF>;
#include "elem2d_march.inl"
}

// CF: 0 nu = 1 and no reaction term, 1 nu = 1 and a constant sigma, 2 a nodal nu and / or sigma
struct HhFamily {
    using Params = HhParams;
    template <int P, int NGP, bool MASK, bool BCF, int FK>
    static void launch(dim3 grid, dim3 block, hipStream_t s, const HhParams& pp) {
        if (pp.nu || pp.sg) hipLaunchKernelGGL((helmholtz2d_kernel<P, NGP, MASK, BCF, FK, 2>), grid, block, 0, s, pp);
        else if (pp.sgconst != 0.f) hipLaunchKernelGGL((helmholtz2d_kernel<P, NGP, MASK, BCF, FK, 1>), grid, block, 0, s, pp);
        else hipLaunchKernelGGL((helmholtz2d_kernel<P, NGP, MASK, BCF, FK, 0>), grid, block, 0, s, pp);
    }
};

#ifndef HH_DEGREE      // helmholtz.hip itself; helmholtz_q2.hip and helmholtz_q3.hip compile the higher degrees
ELEM2D_DEGREE(extern, HhFamily, 2);
ELEM2D_DEGREE(extern, HhFamily, 3);
#else
ELEM2D_DEGREE(, HhFamily, HH_DEGREE);
#endif

}  // namespace dn

#ifndef HH_DEGREE
using namespace dn;

extern "C" int64_t dn_helmholtz_workspace_bytes(const dn_mesh* m) {
    if (elem2d_validate(m) != 0) return DN_E_BADARG;
    return elem2d_workspace_bytes(m, 2);
}

extern "C" int dn_helmholtz_apply(const dn_mesh* m, const dn_helmholtz_args* a, void* stream) {
    int rc = elem2d_validate(m);
    if (rc) return rc;
    if (!a || !a->u) return DN_E_BADARG;
    if (!a->out && !a->energy && !a->sumsq) return DN_E_BADARG;
    if ((a->nu_batched | a->sigma_batched) & ~1) return DN_E_BADARG;
    const bool sums = a->energy || a->sumsq;
    if ((rc = elem2d_check_args(m, a, sums ? 2 : 0))) return rc;
    const Elem2dGeom g = elem2d_plan(m);

    HhParams pp;
    elem2d_fill(pp, m, a, g, sums);
    pp.c = a->c; pp.cr = a->cr; pp.fs = a->fs; pp.alpha = a->alpha; pp.gamma = a->gamma; pp.beta = a->beta;
    pp.sgconst = a->sigma ? 0.f : a->sigma_value;
    pp.fconst = (a->f || a->f_gp) ? 0.f : a->f_value;
    pp.out_scale = a->out_scale;
    pp.u = a->u; pp.nu = a->nu; pp.sg = a->sigma; pp.nu_batched = a->nu_batched; pp.sg_batched = a->sigma_batched;
    pp.out = a->out;
    pp.energy = a->energy;
    pp.sumsq = a->sumsq;
    elem2d_launch<HhFamily>(m, pp, g, reinterpret_cast<hipStream_t>(stream));
    DN_LAUNCH_CHECK();
    return 0;
}
#endif
