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
#include "elem2d_common.h"      // everything the kernel shares with fosls.hip and helmholtz.hip: parameters, the march, plan, checks, launch switch

namespace dn {

struct SfParams : Elem2dParams {
    float dxx[4][4], dyy[4][4];            // second derivatives (scaled by (2/h)^2)
    float ax, ay, bb, cxx, cyy, fs, fconst, out_scale;
    const float* u;
    const float* in_scale;
    float* grad;
    double* sum;
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

// What the march (elem2d_march.inl) asks of the operator: one field, one sum
template <int P_, int NGP_, int FK_, bool NL, bool D2>
struct SfOp {
    static constexpr int P = P_, NGP = NGP_, FK = FK_, NF = 1, NS = 1, NB = P + 1;
    static constexpr bool FOLDS_OK = false;
    struct Raw { float v[NB]; };
    const float* ub;
    float gscale;
    float cu[NB][NB];

    __device__ __forceinline__ void init(const SfParams& p, int b, int64_t nps) {
        ub = p.u + (int64_t)b * nps;
    }
    __device__ __forceinline__ void start(const SfParams& p) {
        gscale = p.out_scale;
        if (p.in_scale) gscale *= p.in_scale[0];
    }
    __device__ __forceinline__ float* out_base(const SfParams& p, int, int b, int64_t nps) const { return p.grad ? p.grad + (int64_t)b * nps : nullptr; }
    template <class F>
    __device__ __forceinline__ void issue(const SfParams& p, unsigned rowoff, int x0, Raw& w, F issue_f) const {
        load_seg<P, false>(ub, rowoff, x0, p.nx, w.v);
        issue_f();
    }
    __device__ __forceinline__ float raw_u(const Raw& w, int n) const { return w.v[n]; }
    __device__ __forceinline__ void put(const SfParams&, const Raw&, int r, int n, float v) { cu[r][n] = v; }
    __device__ __forceinline__ void shift(int n) { cu[0][n] = cu[P][n]; }
    __device__ __forceinline__ float element(const SfParams& p, const float (&fn)[NB][NB], const float (&fg)[NGP * NGP], float,
                                             float (&g)[1][NB][NB]) const {
        return sf_elem<P, NGP, FK, NL, D2>(p, cu, fn, fg, g[0]);
    }
    // no gradient reaches a Dirichlet node
    __device__ __forceinline__ float finish_row(const SfParams&, int, float (&row)[P], unsigned fixed, int) const {
#pragma unroll
        for (int n = 0; n < P; ++n) {
            const float v = row[n] * gscale;
            row[n] = (fixed & (1u << n)) ? 0.f : v;
        }
        return 0.f;
    }
    __device__ __forceinline__ void write_sums(const SfParams& p, const double (&tot)[1]) const { p.sum[0] = tot[0]; }
};

template <int P, int NGP, bool MASK, bool BCF, int FK, bool NL, bool D2>
__global__ void __launch_bounds__(256) strongform2d_kernel(const SfParams p) {
    static_assert(!(D2 && P == 1), "the second derivatives of a Q1 field vanish");
    using Op = SfOp<P, NGP, FK, NL, D2>;
#include "elem2d_march.inl"
}

// NL: b != 0; D2: a second-order term present (Q1: identically zero, no work spent on them)
struct SfFamily {
    using Params = SfParams;
    template <int P, int NGP, bool MASK, bool BCF, int FK>
    static void launch(dim3 grid, dim3 block, hipStream_t s, const SfParams& pp) {
        const bool nl = pp.bb != 0.f;
        if constexpr (P > 1) {
            if (pp.cxx != 0.f || pp.cyy != 0.f) {
                if (nl) hipLaunchKernelGGL((strongform2d_kernel<P, NGP, MASK, BCF, FK, true, true>), grid, block, 0, s, pp);
                else hipLaunchKernelGGL((strongform2d_kernel<P, NGP, MASK, BCF, FK, false, true>), grid, block, 0, s, pp);
                return;
            }
        }
        if (nl) hipLaunchKernelGGL((strongform2d_kernel<P, NGP, MASK, BCF, FK, true, false>), grid, block, 0, s, pp);
        else hipLaunchKernelGGL((strongform2d_kernel<P, NGP, MASK, BCF, FK, false, false>), grid, block, 0, s, pp);
    }
};

#ifndef SF_DEGREE      // strongform.hip itself; strongform_q2.hip and strongform_q3.hip compile the higher degrees
ELEM2D_DEGREE(extern, SfFamily, 2);
ELEM2D_DEGREE(extern, SfFamily, 3);
#else
ELEM2D_DEGREE(, SfFamily, SF_DEGREE);
#endif

}  // namespace dn

#ifndef SF_DEGREE
using namespace dn;

extern "C" int64_t dn_strongform_workspace_bytes(const dn_mesh* m) {
    if (elem2d_validate(m) != 0) return DN_E_BADARG;
    return elem2d_workspace_bytes(m, 1);
}

extern "C" int dn_strongform_apply(const dn_mesh* m, const dn_strongform_args* a, void* stream) {
    int rc = elem2d_validate(m);
    if (rc) return rc;
    if (!a || !a->u) return DN_E_BADARG;
    if (!a->grad && !a->sum) return DN_E_BADARG;
    if ((rc = elem2d_check_args(m, a, a->sum ? 1 : 0))) return rc;
    const Elem2dGeom g = elem2d_plan(m);

    SfParams pp;
    elem2d_fill(pp, m, a, g, a->sum != nullptr);
    const double sx = m->scale[0], sy = m->scale[1];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const bool in = i < m->ngp && j <= m->degree;
            pp.dxx[i][j] = in ? (float)(a->d2basis[i][j] * sx * sx) : 0.f;
            pp.dyy[i][j] = in ? (float)(a->d2basis[i][j] * sy * sy) : 0.f;
        }
    pp.ax = a->ax; pp.ay = a->ay; pp.bb = a->b; pp.cxx = a->dxx; pp.cyy = a->dyy; pp.fs = a->fs;
    pp.fconst = (a->f || a->f_gp) ? 0.f : a->f_value;
    pp.out_scale = a->out_scale;
    pp.u = a->u;
    pp.in_scale = a->in_scale;
    pp.grad = a->grad;
    pp.sum = a->sum;
    elem2d_launch<SfFamily>(m, pp, g, reinterpret_cast<hipStream_t>(stream));
    DN_LAUNCH_CHECK();
    return 0;
}
#endif
