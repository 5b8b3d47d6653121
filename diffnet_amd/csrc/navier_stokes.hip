// Fused 2-D Navier-Stokes (VMS) residuals on Q1 meshes and their VJP: dn_ns_apply (include/diffnet_hip.h).
//
// The nonlinear residual body of examples/navier-stokes/single_instance/e1_ns_ldc_resmin.py:147-308 of the reference (calc_tau,
// calc_residuals) and of e2_ns_fps_resmin.py:293 calc_residuals_ns and its siblings: Dirichlet substitution of u, v, p, the Gauss-point
// evaluations, the variational-multiscale weak forms with the detached stabilisation parameters tau_m / tau_c, their assembly, the Dirichlet
// rows (which take the boundary VALUE) and the three sums of squares -- in one launch.
//
// Flux form: at a Gauss point every weak form is  T_k,a = N_a A_k + Nx_a B_k + Ny_a C_k  with nine pointwise coefficients
//     A1 = a1 - f1 - tm (r1 u_x + r2 u_y)    B1 = visco u_x - p + tm u r1 - tm^2 r1 r1 + tc d    C1 = visco u_y + tm v r1 - tm^2 r1 r2
//     A2 = a2 - f2 - tm (r1 v_x + r2 v_y)    B2 = visco v_x + tm u r2 - tm^2 r2 r1               C2 = visco v_y - p + tm v r2 - tm^2 r2 r2 + tc d
//     A3 = d                                 B3 = tm r1                                          C3 = tm r2
// (a1 = u u_x + v u_y, a2 = u v_x + v v_y, d = u_x + v_y, r1 = a1 + p_x - f1, r2 = a2 + p_y - f2).  The VJP mode has the same form: with the
// cotangents evaluated like fields (L_k, L_k,x, L_k,y) the pullback of s = sum_k (L_k A_k + L_k,x B_k + L_k,y C_k) with tau held fixed is
// again N_a G + Nx_a G_x + Ny_a G_y per field (ns_vjp_flux below; DESIGN.md section 3.2 has the derivation), so both modes share the march.
//
// The mapping is the element-owner march of q1_owner_march.h (one wave = 62 owner columns + two ghost lanes, every output node written
// once by its owner lane with the same additions in any launch plan); the kernel supplies its rows, its element and its Dirichlet-row
// rule.  Sums of squares: fixed-order fp64 reduction (finish_sums3).
#include "flow2d_common.h"      // everything the kernel shares with stokes.hip: parameters, lane set-up, row loader, plan, checks, launch switch

namespace dn {

struct NsParams : Flow2dParams {
    Q1Tables tb;
    float visco;
    float Gx, Gy, diff, gg_inv;            // tau: Gx = 4 / hx^2, Gy = 4 / hy^2, diff = cinv visco^2 (Gx^2 + Gy^2), gg_inv = 1 / (gx^2 + gy^2)
    const float* cot[3];                   // VJP: the cotangents of R1..R3 (fld: the linearisation point)
};

// A landed node row: substituted values of the lane's node (c) and of its right neighbour (n); VJP: the cotangents likewise
template <bool VJP>
struct NsRow {
    float c[3], n[3];
    float lc[VJP ? 3 : 1] = {}, ln[VJP ? 3 : 1] = {};      // the forward does not set them
    unsigned fixed;
    float bv[3];
};

// forward coefficients (A, B, C) of the three weak forms at a point
__device__ __forceinline__ void ns_fwd_flux(const NsParams& p, float u, float ux, float uy, float v, float vx, float vy, float pg, float px,
                                            float py, float f1, float f2, float (&A)[3], float (&B)[3], float (&Cc)[3]) {
    const float a1 = fmaf(u, ux, v * uy), a2 = fmaf(u, vx, v * vy), d = ux + vy;
    const float r1 = a1 + px - f1, r2 = a2 + py - f2;
    const float temp = sqrtf(fmaf(p.Gx, u * u, p.Gy * (v * v)) + p.diff);     // calc_tau; tau is detached
    const float tm = 1.f / temp, tc = temp * p.gg_inv, tm2 = tm * tm;
    const float tr1 = tm * r1, tr2 = tm * r2, qr1 = tm2 * r1, qr2 = tm2 * r2;
    A[0] = a1 - f1 - tm * fmaf(r1, ux, r2 * uy);
    B[0] = fmaf(p.visco, ux, -pg) + fmaf(u, tr1, -qr1 * r1) + tc * d;
    Cc[0] = fmaf(p.visco, uy, fmaf(v, tr1, -qr1 * r2));
    A[1] = a2 - f2 - tm * fmaf(r1, vx, r2 * vy);
    B[1] = fmaf(p.visco, vx, fmaf(u, tr2, -qr2 * r1));
    Cc[1] = fmaf(p.visco, vy, -pg) + fmaf(v, tr2, -qr2 * r2) + tc * d;
    A[2] = d;
    B[2] = tr1;
    Cc[2] = tr2;
}

// VJP coefficients: d/d(u, u_x, u_y | v, v_x, v_y | p, p_x, p_y) of sum_k (L_k A_k + Lx_k B_k + Ly_k C_k), tau held fixed
__device__ __forceinline__ void ns_vjp_flux(const NsParams& p, float u, float ux, float uy, float v, float vx, float vy, float px, float py,
                                            float f1, float f2, const float (&L)[3], const float (&Lx)[3], const float (&Ly)[3],
                                            float (&A)[3], float (&B)[3], float (&Cc)[3]) {
    const float a1 = fmaf(u, ux, v * uy), a2 = fmaf(u, vx, v * vy);
    const float r1 = a1 + px - f1, r2 = a2 + py - f2;
    const float temp = sqrtf(fmaf(p.Gx, u * u, p.Gy * (v * v)) + p.diff);
    const float tm = 1.f / temp, tc = temp * p.gg_inv, tm2 = tm * tm;
    const float tu = tm * u, tv = tm * v, qr1 = tm2 * r1, qr2 = tm2 * r2;
    // partials with respect to the strong residuals r1, r2 (r1 = a1 + p_x - f1: also the p_x, p_y coefficients)
    const float g1 = -tm * fmaf(L[0], ux, L[1] * vx) + Lx[0] * (tu - 2.f * qr1) + Ly[0] * (tv - qr2) - Lx[1] * qr2 + Lx[2] * tm;
    const float g2 = -tm * fmaf(L[0], uy, L[1] * vy) - Ly[0] * qr1 + Lx[1] * (tu - qr1) + Ly[1] * (tv - 2.f * qr2) + Ly[2] * tm;
    const float h1 = L[0] + g1, h2 = L[1] + g2;                         // with respect to a1, a2
    const float hd = fmaf(tc, Lx[0] + Ly[1], L[2]);                     // with respect to d
    A[0] = fmaf(h1, ux, h2 * vx) + tm * fmaf(Lx[0], r1, Lx[1] * r2);
    B[0] = fmaf(h1, u, -tm * r1 * L[0]) + fmaf(p.visco, Lx[0], hd);
    Cc[0] = fmaf(h1, v, -tm * r2 * L[0]) + p.visco * Ly[0];
    A[1] = fmaf(h1, uy, h2 * vy) + tm * fmaf(Ly[0], r1, Ly[1] * r2);
    B[1] = fmaf(h2, u, -tm * r1 * L[1]) + p.visco * Lx[1];
    Cc[1] = fmaf(h2, v, -tm * r2 * L[1]) + fmaf(p.visco, Ly[1], hd);
    A[2] = -(Lx[0] + Ly[1]);
    B[2] = g1;
    Cc[2] = g2;
}

template <int NGP, bool MASK, bool BCF, bool FGP, bool VJP>
__global__ void __launch_bounds__(256) ns2d_kernel(const NsParams p) {
    constexpr int G = NGP * NGP;
    int lane, chunk, strip;
    flow2d_wave(p, lane, chunk, strip);

    __shared__ double red[16];
    __shared__ int last_flag;
    float sq[3] = {0.f, 0.f, 0.f};

    if (strip < p.strips) {
        const int nx = p.nx, ny = p.ny;
        constexpr int NX = VJP ? 3 : 0;             // a row of the VJP carries the three cotangents
        Flow2dLane<NX> L;
        flow2d_lane(p, chunk, lane, L);
        const int b = blockIdx.y;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            flow2d_field_base<G>(p, b, k, L);
            if constexpr (VJP) L.xb[k] = p.cot[k] + (int64_t)b * ((int64_t)nx * ny);
        }

        float lscale[3] = {1.f, 1.f, 1.f};
        if constexpr (VJP) flow2d_in_scale(p, lscale);       // in_num / in_den scales the cotangents

        using Raw = Flow2dRaw<G, MASK, BCF, FGP, NX>;
        using Row = NsRow<VJP>;
        auto issue = [&](int r, Raw& w) { flow2d_issue(p, L, r, w); };

        // Dirichlet substitution of a landed row (the cotangent of a Dirichlet row is zero) and the right neighbours
        auto consume = [&](const Raw& w, Row& R) {
            R.fixed = 0u;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float val = w.v[k];
                float lv = 0.f;
                if constexpr (VJP) lv = w.x[k] * lscale[k];
                R.bv[k] = p.bcv[k];
                if constexpr (MASK) {
                    const bool fx = flow2d_fixed(p, w, k);
                    if constexpr (BCF) R.bv[k] = p.bcf[k] ? w.bf[k] : R.bv[k];
                    val = fx ? R.bv[k] : val;
                    lv = fx ? 0.f : lv;
                    R.fixed |= fx ? (1u << k) : 0u;
                }
                R.c[k] = val;
                R.n[k] = __shfl_down(val, 1, 64);
                if constexpr (VJP) {
                    R.lc[k] = lv;
                    R.ln[k] = __shfl_down(lv, 1, 64);
                }
            }
        };

        // the lane's element in element row e (node rows e, e + 1: Bm, Tp): its four local contributions per weak form, zero where the
        // element does not exist; returns the parts that belong to the lane's node in rows e (bot) and e + 1 (top)
        auto element = [&](const Row& Bm, const Row& Tp, const Raw& w, int e, float (&bot)[3], float (&top)[3]) {
            float acc[3][4];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int a = 0; a < 4; ++a) acc[k][a] = 0.f;
#pragma unroll
            for (int jg = 0; jg < NGP; ++jg) {
                const float by0 = p.tb.by[jg][0], by1 = p.tb.by[jg][1], dy0 = p.tb.dy[jg][0], dy1 = p.tb.dy[jg][1];
#pragma unroll
                for (int ig = 0; ig < NGP; ++ig) {
                    const int g = jg * NGP + ig;
                    const float bx0 = p.tb.bx[ig][0], bx1 = p.tb.bx[ig][1], dx0 = p.tb.dx[ig][0], dx1 = p.tb.dx[ig][1];
                    float val[3], gx[3], gy[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        q1_eval(bx0, bx1, dx0, dx1, by0, by1, dy0, dy1, Bm.c[k], Bm.n[k], Tp.c[k], Tp.n[k], val[k], gx[k], gy[k]);
                    float f1 = p.fconst[0], f2 = p.fconst[1];
                    if constexpr (FGP) {
                        f1 = p.fgp[0] ? w.f[0][g] : f1;
                        f2 = p.fgp[1] ? w.f[1][g] : f2;
                    }
                    float A[3], Bc[3], Cc[3];
                    if constexpr (VJP) {
                        float L[3], Lx[3], Ly[3];
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            q1_eval(bx0, bx1, dx0, dx1, by0, by1, dy0, dy1, Bm.lc[k], Bm.ln[k], Tp.lc[k], Tp.ln[k], L[k], Lx[k], Ly[k]);
                        ns_vjp_flux(p, val[0], gx[0], gy[0], val[1], gx[1], gy[1], gx[2], gy[2], f1, f2, L, Lx, Ly, A, Bc, Cc);
                    } else {
                        ns_fwd_flux(p, val[0], gx[0], gy[0], val[1], gx[1], gy[1], val[2], gx[2], gy[2], f1, f2, A, Bc, Cc);
                    }
                    const float wq = p.tb.wg[g];
#pragma unroll
                    for (int k = 0; k < 3; ++k) q1_flux_scatter(bx0, bx1, dx0, dx1, by0, by1, dy0, dy1, wq, A[k], Bc[k], Cc[k], acc[k]);
                }
            }
            const bool ok = L.elem_x && e >= 0 && e < p.nely;
#pragma unroll
            for (int k = 0; k < 3; ++k) q1_owner_handover(ok, acc[k], bot[k], top[k]);
        };

        // node row e of the three residuals
        auto finish = [&](int e, const Row& R, const float (&carry)[3], const float (&bot)[3]) {
            const unsigned rowoff = (unsigned)e * (unsigned)nx + L.qc;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float r = carry[k] + bot[k];
                if constexpr (MASK) {
                    // forward: Dirichlet rows take the boundary value (the scripts' torch.where); VJP: no gradient reaches a substituted node
                    const bool fx = (R.fixed & (1u << k)) != 0u;
                    r = fx ? (VJP ? 0.f : R.bv[k]) : r;
                }
                sq[k] = L.owner ? fmaf(r, r, sq[k]) : sq[k];
                if (L.owner && L.ob[k]) st_at<float>(L.ob[k], rowoff, r);
            }
        };

        const int j0 = strip * p.rows_per_strip, j1 = min(j0 + p.rows_per_strip, ny);
        constexpr int NF = 3;
#include "q1_owner_march.inl"
    }
    if (p.want_sums) finish_sums3(p.part, p.counter, p.sumsq, p.norms, sq, (int)threadIdx.x, (int)blockDim.x, red, &last_flag);
}

template <int NGP, bool VJP>
struct NsFamily {
    template <bool MASK, bool BCF, bool FGP>
    static void launch(dim3 grid, dim3 block, hipStream_t s, const NsParams& pp) {
        hipLaunchKernelGGL((ns2d_kernel<NGP, MASK, BCF, FGP, VJP>), grid, block, 0, s, pp);
    }
};

template <int NGP>
static void ns_launch_ngp(const NsParams& pp, const Flow2dGeom& g, int batch, bool vjp, hipStream_t s) {
    if (vjp) flow2d_launch<NsFamily<NGP, true>>(pp, g, batch, s);
    else flow2d_launch<NsFamily<NGP, false>>(pp, g, batch, s);
}

constexpr int NS_MIN_ROWS = 8;          // shortest strip (flow2d_plan): a strip recomputes one halo element row

}  // namespace dn

using namespace dn;

extern "C" int64_t dn_ns_workspace_bytes(const dn_mesh* m) {
    if (flow2d_validate(m) != 0) return DN_E_BADARG;
    return flow2d_workspace_bytes(flow2d_plan(m, NS_MIN_ROWS), m->batch);
}

extern "C" int dn_ns_apply(const dn_mesh* m, const dn_ns_args* a, void* stream) {
    int rc = flow2d_validate(m);
    if (rc) return rc;
    if ((rc = flow2d_check_args(a))) return rc;
    if (a->vjp & ~1) return DN_E_BADARG;
    const bool vjp = a->vjp != 0;
    if (vjp && (!a->cot[0] || !a->cot[1] || !a->cot[2])) return DN_E_BADARG;     // a VJP without its cotangents
    if (!vjp && a->in_num) return DN_E_BADARG;                                    // the scaling applies to the cotangents only
    if (!(a->tau_h[0] > 0.f) || !(a->tau_h[1] > 0.f)) return DN_E_BADARG;
    const Flow2dGeom g = flow2d_plan(m, NS_MIN_ROWS);
    if ((rc = flow2d_check_workspace(a, g, m->batch))) return rc;

    NsParams pp;
    const int ngp = m->ngp;
    q1_tables_fill(pp.tb, m, a->wscale);
    // calc_tau of the scripts: g and G are float32 tensors, the diffusion part a float32 product
    const float visco = a->visco;
    const double hx = a->tau_h[0], hy = a->tau_h[1];
    const float gx = (float)(2.0 / hx), gy = (float)(2.0 / hy);
    const float Gx = (float)(4.0 / (hx * hx)), Gy = (float)(4.0 / (hy * hy));
    pp.visco = visco;
    pp.Gx = Gx;
    pp.Gy = Gy;
    pp.diff = (float)((double)a->cinv * (double)visco * (double)visco) * (Gx * Gx + Gy * Gy);
    pp.gg_inv = 1.f / (gx * gx + gy * gy);
    flow2d_fill(pp, m, a, g);
    for (int k = 0; k < 3; ++k) pp.cot[k] = vjp ? a->cot[k] : nullptr;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (ngp) {
        case 2: ns_launch_ngp<2>(pp, g, m->batch, vjp, s); break;
        case 3: ns_launch_ngp<3>(pp, g, m->batch, vjp, s); break;
        default: ns_launch_ngp<4>(pp, g, m->batch, vjp, s); break;
    }
    DN_LAUNCH_CHECK();
    return 0;
}
