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
#include "elem2d_common.h"      // everything the kernel shares with strongform.hip and helmholtz.hip: parameters, the march, plan, checks, launch switch

namespace dn {

struct FoParams : Elem2dParams {
    float wq, wd, fs, fconst, nuconst, out_scale;
    const float* fld[3];                   // u, mx, my
    int64_t fld_stride, grad_stride;       // elements between samples
    const float* nu;                       // NUF: nodal coefficient
    int nu_batched;
    const float* in_scale;
    float* grad[3];
    double* sum;
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

// What the march (elem2d_march.inl) asks of the operator: three fields (one barrier per node row for the three), one sum
template <int P_, int NGP_, int FK_, bool NUF>
struct FoOp {
    static constexpr int P = P_, NGP = NGP_, FK = FK_, NF = 3, NS = 1, NB = P + 1;
    static constexpr bool FOLDS_OK = true;      // fo_elem folds `ok` into the weights
    struct Raw { float v[3][NB], c[NUF ? NB : 1]; };
    const float* ub;
    const float* fldb[3];
    const float* nub;
    float gscale;
    float cu[3][NB][NB], cn[NB][NB];

    __device__ __forceinline__ void init(const FoParams& p, int b, int64_t nps) {
#pragma unroll
        for (int k = 0; k < 3; ++k) fldb[k] = p.fld[k] + (int64_t)b * p.fld_stride;
        ub = fldb[0];
        nub = NUF ? p.nu + (p.nu_batched ? (int64_t)b * nps : 0) : ub;
    }
    __device__ __forceinline__ void start(const FoParams& p) {
        gscale = p.out_scale;
        if (p.in_scale) gscale *= p.in_scale[0];
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int n = 0; n < NB; ++n) cn[r][n] = 0.f;
    }
    __device__ __forceinline__ float* out_base(const FoParams& p, int k, int b, int64_t) const {
        return p.grad[k] ? p.grad[k] + (int64_t)b * p.grad_stride : nullptr;
    }
    template <class F>
    __device__ __forceinline__ void issue(const FoParams& p, unsigned rowoff, int x0, Raw& w, F issue_f) const {
#pragma unroll
        for (int k = 0; k < 3; ++k) load_seg<P, false>(fldb[k], rowoff, x0, p.nx, w.v[k]);
        if constexpr (NUF) load_seg<P, false>(nub, rowoff, x0, p.nx, w.c);
        issue_f();
    }
    __device__ __forceinline__ float raw_u(const Raw& w, int n) const { return w.v[0][n]; }
    // mx and my are free
    __device__ __forceinline__ void put(const FoParams&, const Raw& w, int r, int n, float v) {
        cu[0][r][n] = v;
        cu[1][r][n] = w.v[1][n];
        cu[2][r][n] = w.v[2][n];
        if constexpr (NUF) cn[r][n] = w.c[n];
    }
    __device__ __forceinline__ void shift(int n) {
        cn[0][n] = cn[P][n];
#pragma unroll
        for (int k = 0; k < 3; ++k) cu[k][0][n] = cu[k][P][n];
    }
    __device__ __forceinline__ float element(const FoParams& p, const float (&fn)[NB][NB], const float (&fg)[NGP * NGP], float okf,
                                             float (&acc)[3][NB][NB]) const {
        return fo_elem<P, NGP, FK, NUF>(p, cu, cn, fn, fg, okf, acc);
    }
    // no gradient of u reaches a Dirichlet node
    __device__ __forceinline__ float finish_row(const FoParams&, int k, float (&row)[P], unsigned fixed, int) const {
#pragma unroll
        for (int n = 0; n < P; ++n) {
            float v = row[n] * gscale;
            if (k == 0) v = (fixed & (1u << n)) ? 0.f : v;
            row[n] = v;
        }
        return 0.f;
    }
    __device__ __forceinline__ void write_sums(const FoParams& p, const double (&tot)[1]) const { p.sum[0] = tot[0]; }
};

template <int P, int NGP, bool MASK, bool BCF, int FK, bool NUF>
__global__ void __launch_bounds__(256) fosls2d_kernel(const FoParams p) {
    using Op = FoOp<P, NGP, FK, NUF>;
#include "elem2d_march.inl"
}

struct FoFamily {
    using Params = FoParams;
    template <int P, int NGP, bool MASK, bool BCF, int FK>
    static void launch(dim3 grid, dim3 block, hipStream_t s, const FoParams& pp) {
        if (pp.nu) hipLaunchKernelGGL((fosls2d_kernel<P, NGP, MASK, BCF, FK, true>), grid, block, 0, s, pp);
        else hipLaunchKernelGGL((fosls2d_kernel<P, NGP, MASK, BCF, FK, false>), grid, block, 0, s, pp);
    }
};

#ifndef FO_DEGREE      // fosls.hip itself; fosls_q2.hip and fosls_q3.hip compile the higher degrees
ELEM2D_DEGREE(extern, FoFamily, 2);
ELEM2D_DEGREE(extern, FoFamily, 3);
#else
ELEM2D_DEGREE(, FoFamily, FO_DEGREE);
#endif

}  // namespace dn

#ifndef FO_DEGREE
using namespace dn;

extern "C" int64_t dn_fosls_workspace_bytes(const dn_mesh* m) {
    if (elem2d_validate(m) != 0) return DN_E_BADARG;
    return elem2d_workspace_bytes(m, 1);
}

extern "C" int dn_fosls_apply(const dn_mesh* m, const dn_fosls_args* a, void* stream) {
    int rc = elem2d_validate(m);
    if (rc) return rc;
    if (!a || !a->u || !a->mx || !a->my) return DN_E_BADARG;
    const bool any_grad = a->grad_u || a->grad_mx || a->grad_my;
    if (!any_grad && !a->sum) return DN_E_BADARG;
    const int64_t nps = (int64_t)m->nx * m->ny;
    if (a->field_stride < nps || (any_grad && a->grad_stride < nps)) return DN_E_BADARG;
    if (a->nu_batched & ~1) return DN_E_BADARG;
    if ((rc = elem2d_check_args(m, a, a->sum ? 1 : 0))) return rc;
    const Elem2dGeom g = elem2d_plan(m);

    FoParams pp;
    elem2d_fill(pp, m, a, g, a->sum != nullptr);
    pp.wq = a->wq; pp.wd = a->wd; pp.fs = a->fs;
    pp.fconst = (a->f || a->f_gp) ? 0.f : a->f_value;
    pp.nuconst = a->nu ? 0.f : a->nu_value;
    pp.out_scale = a->out_scale;
    pp.fld[0] = a->u; pp.fld[1] = a->mx; pp.fld[2] = a->my;
    pp.fld_stride = a->field_stride; pp.grad_stride = any_grad ? a->grad_stride : 0;
    pp.nu = a->nu; pp.nu_batched = a->nu_batched;
    pp.in_scale = a->in_scale;
    pp.grad[0] = a->grad_u; pp.grad[1] = a->grad_mx; pp.grad[2] = a->grad_my;
    pp.sum = a->sum;
    elem2d_launch<FoFamily>(m, pp, g, reinterpret_cast<hipStream_t>(stream));
    DN_LAUNCH_CHECK();
    return 0;
}
#endif
