// Fused 2-D stabilised eikonal weak-form residual on structured Q_P meshes and its VJP: dn_eikonal_apply (include/diffnet_hip.h).
//
// The domain term of the eikonal scripts of the reference, examples/eiqonal/parametric/10_fixed_bc.py:127-216 (loss_eikonal) and
// examples/eiqonal/single_instance/e01_curve_reconstruction.py:452-558 (loss4): the two Dirichlet substitutions, the Gauss-point
// evaluations of u, u_x and u_y, the stabilised weak form, its assembly, the zeroed Dirichlet rows and the Frobenius norm -- in one launch.
//
//   R_a   = zero_on_dirichlet( sum_{e contains a} sum_g W_g ( tau u~_g gradN_a . grad u~_g + sq N_a |grad u~_g|^2 - N_a f_g ) ),  W_g = gpw_g wscale
//   sumsq = sum over (b, nodes) of R^2,   norm = sqrt(sumsq)
//
// Flux form: at a Gauss point the weak form is  T_a = N_a A + Nx_a B + Ny_a C  with
//     A = sq (u_x^2 + u_y^2) - f      B = tau u u_x      C = tau u u_y
// The VJP mode has the same form: with the cotangent (zero on the Dirichlet nodes) evaluated like a field (L, L_x, L_y)
//     A' = tau (L_x u_x + L_y u_y)      B' = 2 sq L u_x + tau u L_x      C' = 2 sq L u_y + tau u L_y
// so both modes share the element (DESIGN.md section 3.2 has the derivation).  The VJP reads u and the cotangent, never the forcing.
//
// Same mapping as the Helmholtz kernel (helmholtz.hip; the element form of fsdt.hip has the reasons): a thread owns one element column of
// a strip and marches over element rows; the element is sum-factorised one x-Gauss point at a time (forward: u, u_x, u_y and the nodal
// forcing, in the VJP the cotangent likewise; transposed: the three flux coefficients W A | W B | W C on N | Nx | Ny); the contribution
// to the node column shared with the right neighbour goes through a double-buffered LDS slot; strip and chunk seams are closed by
// recomputing one layer / one column.  No atomics on the data path: every node is written once, by its owner, with the same additions
// in the same order under any launch plan and batch size.  sumsq counts every node once (its owner, after its value is complete): per
// node row in fp32, per thread in fp64, then the fixed-order fp64 reduction of dn_reduce.h.
//
// Optional inputs are compile-time forms: MASK (any condition), BCF (any value field), FK (forcing: constant / nodal / at the Gauss
// points; the VJP has FK == 0 only), VJP.  12 forms per (degree, rule).
#include "elem2d_common.h"      // everything the kernel shares with strongform.hip, fosls.hip and helmholtz.hip

namespace dn {

struct EkParams : Elem2dParams {
    float tau, sq, sq2, fconst;            // sq2 = 2 sq
    const float* u;
    const float* cot;                      // VJP: the cotangent of R (u: the linearisation point)
    const float* in_num;                   // VJP: cot is scaled by in_num[0] (/ in_den[0])
    const float* in_den;
    int vjp;
    float* out;
    double* sumsq;                         // sum 1: every node once (its owner, after its value is complete)
    float* norm;                           // its square root
};

// One element: nodal values F[jb][ib] of u~ (Ln: the cotangent, Fn: the nodal forcing); its contributions to out are ADDED to g[jb][ib].
// fg: the forcing at the element's Gauss points (FK == 2).
template <int P, int NGP, int FK, bool VJP>
__device__ __forceinline__ void ek_elem(const EkParams& p, const float (&F)[P + 1][P + 1], const float (&Ln)[P + 1][P + 1],
                                        const float (&Fn)[P + 1][P + 1], const float (&fg)[NGP * NGP], float (&g)[P + 1][P + 1]) {
    constexpr int NB = P + 1;
#pragma unroll
    for (int ig = 0; ig < NGP; ++ig) {
        float tv[NB], td[NB], tl[NB], tm[NB], tf[NB], rv[NB], rd[NB];
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
            float a = 0.f, d = 0.f, l = 0.f, m = 0.f, ff = 0.f;
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) {
                a = fmaf(p.b[ig][ib], F[jb][ib], a);
                d = fmaf(p.dx[ig][ib], F[jb][ib], d);
                if constexpr (VJP) {
                    l = fmaf(p.b[ig][ib], Ln[jb][ib], l);
                    m = fmaf(p.dx[ig][ib], Ln[jb][ib], m);
                }
                if constexpr (FK == 1) ff = fmaf(p.b[ig][ib], Fn[jb][ib], ff);
            }
            tv[jb] = a; td[jb] = d; tl[jb] = l; tm[jb] = m; tf[jb] = ff;
            rv[jb] = 0.f; rd[jb] = 0.f;
        }
#pragma unroll
        for (int jg = 0; jg < NGP; ++jg) {
            float v = 0.f, ux = 0.f, uy = 0.f, L = 0.f, Lx = 0.f, Ly = 0.f, f = p.fconst;
            if constexpr (FK == 1) f = 0.f;
            if constexpr (FK == 2) f = fg[jg * NGP + ig];
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
                v = fmaf(p.b[jg][jb], tv[jb], v);
                ux = fmaf(p.b[jg][jb], td[jb], ux);
                uy = fmaf(p.dy[jg][jb], tv[jb], uy);
                if constexpr (VJP) {
                    L = fmaf(p.b[jg][jb], tl[jb], L);
                    Lx = fmaf(p.b[jg][jb], tm[jb], Lx);
                    Ly = fmaf(p.dy[jg][jb], tl[jb], Ly);
                }
                if constexpr (FK == 1) f = fmaf(p.b[jg][jb], tf[jb], f);
            }
            const float W = p.w2[jg][ig];
            const float tv_ = p.tau * v;
            float A, Bc, Cc;
            if constexpr (VJP) {
                const float s2L = p.sq2 * L;
                A = p.tau * fmaf(Lx, ux, Ly * uy);
                Bc = fmaf(s2L, ux, tv_ * Lx);
                Cc = fmaf(s2L, uy, tv_ * Ly);
            } else {
                A = fmaf(p.sq, fmaf(ux, ux, uy * uy), -f);
                Bc = tv_ * ux;
                Cc = tv_ * uy;
            }
            const float cn = W * A, cx = W * Bc, cy = W * Cc;
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
}

// What the march (elem2d_march.inl) asks of the operator: one field, two sums (the first unused: the element has no energy; sumsq).
// In the VJP a row carries two nodal arrays, u~ and the cotangent.
template <int P_, int NGP_, int FK_, bool VJP>
struct EkOp {
    static constexpr int P = P_, NGP = NGP_, FK = FK_, NF = 1, NS = 2, NB = P + 1;
    static constexpr bool FOLDS_OK = false;
    static_assert(!VJP || FK == 0, "the VJP does not read the forcing");
    struct Raw { float v[NB], l[VJP ? NB : 1]; };
    const float* ub;
    const float* lb;
    float lscale;
    float cu[NB][NB], cl[VJP ? NB : 1][VJP ? NB : 1];

    __device__ __forceinline__ void init(const EkParams& p, int b, int64_t nps) {
        ub = p.u + (int64_t)b * nps;
        lb = VJP ? p.cot + (int64_t)b * nps : ub;
    }
    __device__ __forceinline__ void start(const EkParams& p) {
        lscale = 1.f;
        if constexpr (VJP) {
            if (p.in_num) {
                lscale = p.in_num[0];
                if (p.in_den) {                     // the VJP of the norm; torch's convention at ||R|| == 0: zero
                    const float den = p.in_den[0];
                    lscale = den > 0.f ? lscale / den : (den == den ? 0.f : den);
                }
            }
        }
    }
    __device__ __forceinline__ float* out_base(const EkParams& p, int, int b, int64_t nps) const { return p.out ? p.out + (int64_t)b * nps : nullptr; }
    template <class F>
    __device__ __forceinline__ void issue(const EkParams& p, unsigned rowoff, int x0, Raw& w, F issue_f) const {
        load_seg<P, false>(ub, rowoff, x0, p.nx, w.v);
        issue_f();
        if constexpr (VJP) load_seg<P, false>(lb, rowoff, x0, p.nx, w.l);
    }
    __device__ __forceinline__ float raw_u(const Raw& w, int n) const { return w.v[n]; }
    __device__ __forceinline__ void put(const EkParams&, const Raw& w, int r, int n, float v) {
        cu[r][n] = v;
        if constexpr (VJP) cl[r][n] = w.l[n] * lscale;
    }
    // the cotangent of a Dirichlet row is zero, as the forward zeroes those rows (the march calls this after put() of a whole row)
    __device__ __forceinline__ void fixed_row(int r, unsigned bits) {
        if constexpr (VJP) {
#pragma unroll
            for (int n = 0; n < NB; ++n) cl[r][n] = (bits & (1u << n)) ? 0.f : cl[r][n];
        }
    }
    __device__ __forceinline__ void shift(int n) {
        cu[0][n] = cu[P][n];
        if constexpr (VJP) cl[0][n] = cl[P][n];
    }
    __device__ __forceinline__ float element(const EkParams& p, const float (&fn)[NB][NB], const float (&fg)[NGP * NGP], float,
                                             float (&g)[1][NB][NB]) const {
        if constexpr (VJP) ek_elem<P, NGP, FK, true>(p, cu, cl, fn, fg, g[0]);
        else ek_elem<P, NGP, FK, false>(p, cu, cu, fn, fg, g[0]);
        return 0.f;
    }
    // nothing reaches a Dirichlet node (forward: the rows of R are zeroed; VJP: no gradient reaches a substituted node); the row's
    // squares go to sumsq
    __device__ __forceinline__ float finish_row(const EkParams& p, int, float (&row)[P], unsigned fixed, int x0) const {
        float rs = 0.f;
#pragma unroll
        for (int n = 0; n < P; ++n) {
            const float v = (fixed & (1u << n)) ? 0.f : row[n];
            rs = (x0 + n < p.nx) ? fmaf(v, v, rs) : rs;
            row[n] = v;
        }
        return rs;
    }
    __device__ __forceinline__ void write_sums(const EkParams& p, const double (&tot)[2]) const {
        if (p.sumsq) p.sumsq[0] = tot[1];
        if (p.norm) p.norm[0] = (float)sqrt(tot[1]);
    }
};

template <int P, int NGP, bool MASK, bool BCF, int FK, bool VJP>
__global__ void __launch_bounds__(256) eikonal2d_kernel(const EkParams p) {
    using Op = EkOp<P, NGP, FK, VJP>;
#include "elem2d_march.inl"
}

struct EkFamily {
    using Params = EkParams;
    template <int P, int NGP, bool MASK, bool BCF, int FK>
    static void launch(dim3 grid, dim3 block, hipStream_t s, const EkParams& pp) {
        if constexpr (FK == 0) {       // dn_eikonal_apply passes no forcing on to the VJP
            if (pp.vjp) { hipLaunchKernelGGL((eikonal2d_kernel<P, NGP, MASK, BCF, 0, true>), grid, block, 0, s, pp); return; }
        }
        hipLaunchKernelGGL((eikonal2d_kernel<P, NGP, MASK, BCF, FK, false>), grid, block, 0, s, pp);
    }
};

#ifndef EK_DEGREE      // eikonal.hip itself; eikonal_q2.hip and eikonal_q3.hip compile the higher degrees
ELEM2D_DEGREE(extern, EkFamily, 2);
ELEM2D_DEGREE(extern, EkFamily, 3);
#else
ELEM2D_DEGREE(, EkFamily, EK_DEGREE);
#endif

}  // namespace dn

#ifndef EK_DEGREE
using namespace dn;

extern "C" int64_t dn_eikonal_workspace_bytes(const dn_mesh* m) {
    if (elem2d_validate(m) != 0) return DN_E_BADARG;
    return elem2d_workspace_bytes(m, 2);
}

extern "C" int dn_eikonal_apply(const dn_mesh* m, const dn_eikonal_args* a, void* stream) {
    int rc = elem2d_validate(m);
    if (rc) return rc;
    if (!a || !a->u) return DN_E_BADARG;
    if (!a->out && !a->sumsq && !a->norm) return DN_E_BADARG;
    if (a->in_den && !a->in_num) return DN_E_BADARG;
    if (a->vjp & ~1) return DN_E_BADARG;
    const bool vjp = a->vjp != 0;
    if (vjp && !a->cot) return DN_E_BADARG;                                  // a VJP without its cotangent
    if (!vjp && a->in_num) return DN_E_BADARG;                               // the scaling applies to the cotangent only
    const bool sums = a->sumsq || a->norm;
    if ((rc = elem2d_check_args(m, a, sums ? 2 : 0))) return rc;
    const Elem2dGeom g = elem2d_plan(m);

    EkParams pp;
    elem2d_fill(pp, m, a, g, sums);
    if (vjp) { pp.f = nullptr; pp.fgp = nullptr; }                           // the VJP does not read the forcing
    pp.tau = a->tau; pp.sq = a->sq; pp.sq2 = 2.f * a->sq;
    pp.fconst = (a->f || a->f_gp) ? 0.f : a->f_value;
    pp.u = a->u;
    pp.cot = vjp ? a->cot : nullptr;
    pp.in_num = a->in_num; pp.in_den = a->in_den;
    pp.vjp = a->vjp;
    pp.out = a->out;
    pp.sumsq = a->sumsq;
    pp.norm = a->norm;
    elem2d_launch<EkFamily>(m, pp, g, reinterpret_cast<hipStream_t>(stream));
    DN_LAUNCH_CHECK();
    return 0;
}
#endif
