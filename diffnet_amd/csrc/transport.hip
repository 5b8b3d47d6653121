// Fused 2-D scalar transport (SUPG) residual on Q1 meshes and its VJP: dn_transport_apply (include/diffnet_hip.h).
//
// The residual body of three scripts of the reference under examples/poisson/single_instance/: e17_adv_diff_2d_resmin.py:99-171
// (AdvDiff2d.loss), e3_st_mms_resmin.py:97-173 (SpaceTimeHeat.loss_resmin) and e18_allen_cahn_ice_melt.py:77-151 (AllenCahnIceMelt.loss):
// the two Dirichlet substitutions of u, the Gauss-point evaluations, the stabilised weak form, its assembly, the Dirichlet rows (which
// take the boundary VALUE) and the sum of squares -- in one launch.
//
// Flux form: at a Gauss point the weak form is  T_a = N_a A + Nx_a B + Ny_a C  with
//     adv = ax u_x + ay u_y      s = adv - f      r(u) = c0 + c1 u + c2 u^2 + c3 u^3
//     A = s + r(u)      B = kx nu u_x + tau ax s      C = ky nu u_y + tau ay s
// The VJP mode has the same form: with the cotangent evaluated like a field (L, L_x, L_y) and q = L + tau (ax L_x + ay L_y)
//     A' = L r'(u)      B' = ax q + kx nu L_x      C' = ay q + ky nu L_y
// so both modes share the march (DESIGN.md section 3.2 has the derivation).  Without a reaction the VJP does not read u.
//
// The mapping is the element-owner march of q1_owner_march.h with one output (one wave = 62 owner columns + two ghost lanes, every output
// node written once by its owner lane with the same additions in any launch plan); the kernel supplies its rows, its element and its
// Dirichlet-row rule.  Sum of squares: fixed-order fp64 reduction (finish_sums<1> in dn_reduce.h).
//
// Optional inputs are compile-time forms: MASK (any condition), BCF (any value field), NU (nodal coefficient), FGP (Gauss-point forcing),
// REACT (c1..c3 != 0: the cubic in the forward, u in the VJP).
#include "flow2d_common.h"      // the mesh check and the launch plan (nothing of the three-field parameters); through it q1_owner_march.h

namespace dn {

struct TransportParams {
    const float* u;
    const float* nu;                       // NU kernels
    int nu_batched;
    const void* mask[2];
    int mask_kind[2];                      // 0: none, 1: uint8 (!= 0), 2: fp32 (>= 0.5)
    int mask_batched[2];
    const float* bcf[2];
    int bcf_batched[2];
    float bcv[2];
    int r_first_wins;                      // rows of R where both conditions hold: condition 1's value (else condition 2's)
    const float* fgp;                      // (B | 1, G, nely, nelx)
    int fgp_batched;
    float fconst;
    const float* cot;                      // VJP: the cotangent of R (u: the linearisation point)
    const float* in_num;                   // VJP: cot is scaled by in_num[0] (/ in_den[0])
    const float* in_den;
    float* out;
    double* part;                          // [nblocks] partial sums of squares
    unsigned* counter;
    double* sumsq;
    float* norm;
    float ax, ay, kx, ky, tax, tay;        // tax = tau ax, tay = tau ay
    float c0, c1, c2, c3;
    Q1Tables tb;
    int nx, ny, nelx, nely, chunks, rows_per_strip, strips, want_sums;
};

// Raw loads of one node row r (clamped into the mesh) and, with the Gauss-point forcing, of the element layer r - 1 under it
template <int G, bool MASK, bool BCF, bool FGP>
struct TransportRaw {
    float v;                               // u (where the mode reads it)
    float nu;                              // NU
    float x;                               // VJP: the cotangent
    float mf[MASK ? 2 : 1];
    uint8_t mb[MASK ? 2 : 1];
    float bf[BCF ? 2 : 1];
    float f[FGP ? G : 1];
};

// A landed node row: substituted value of the lane's node (c) and of its right neighbour (n), nu and the cotangent likewise
struct TransportRow {
    float c = 0.f, n = 0.f, nuc = 0.f, nun = 0.f, lc = 0.f, ln = 0.f;      // a form sets the ones it reads
    bool fixed = false;
    float bv = 0.f;                        // the value a Dirichlet row of R takes
};

template <int NGP, bool MASK, bool BCF, bool NU, bool FGP, bool REACT, bool VJP>
__global__ void __launch_bounds__(256) transport2d_kernel(const TransportParams p) {
    constexpr int G = NGP * NGP;
    constexpr bool NEEDU = !VJP || REACT;           // the VJP of a linear operator does not read the linearisation point
    static_assert(!(VJP && FGP), "the VJP does not read the forcing");
    static_assert(NEEDU || !BCF, "value fields matter only where u is read");
    int lane, chunk, strip;
    flow2d_wave(p, lane, chunk, strip);

    __shared__ double red[16];
    __shared__ int last_flag;
    float sq[1] = {0.f};

    if (strip < p.strips) {
        const int nx = p.nx, ny = p.ny;
        Q1Lane L;
        q1_lane(chunk, lane, nx, p.nelx, p.nely, L);
        const int b = blockIdx.y;
        const int64_t nps = (int64_t)nx * ny;

        // base pointers of the sample
        const float* ub = p.u + (int64_t)b * nps;
        const float* nub = NU ? p.nu + (p.nu_batched ? (int64_t)b * nps : 0) : ub;
        const float* xb = VJP ? p.cot + (int64_t)b * nps : ub;
        float* ob = p.out ? p.out + (int64_t)b * nps : nullptr;
        const float* fg = FGP ? p.fgp + (p.fgp_batched ? (int64_t)b * G * L.nel : 0) : ub;
        const float* bcfb[2];
        const float* mfp[2];
        const uint8_t* mbp[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            bcfb[k] = p.bcf[k] ? p.bcf[k] + (p.bcf_batched[k] ? (int64_t)b * nps : 0) : ub;
            const int64_t mo = p.mask_batched[k] ? (int64_t)b * nps : 0;
            mfp[k] = reinterpret_cast<const float*>(p.mask[k]) + (p.mask_kind[k] == 2 ? mo : 0);
            mbp[k] = reinterpret_cast<const uint8_t*>(p.mask[k]) + (p.mask_kind[k] == 1 ? mo : 0);
        }

        float lscale = 1.f;
        if constexpr (VJP) {
            if (p.in_num) {
                lscale = p.in_num[0];
                if (p.in_den) {                     // the VJP of the norm; torch's convention at ||R|| == 0: zero
                    const float den = p.in_den[0];
                    lscale = den > 0.f ? lscale / den : (den == den ? 0.f : den);
                }
            }
        }

        using Raw = TransportRaw<G, MASK, BCF, FGP>;
        using Row = TransportRow;

        auto issue = [&](int r, Raw& w) {
            const unsigned rowoff = (unsigned)min(max(r, 0), ny - 1) * (unsigned)nx + L.qc;
            if constexpr (NEEDU) w.v = ld_at<float>(ub, rowoff);
            if constexpr (NU) w.nu = ld_at<float>(nub, rowoff);
            if constexpr (VJP) w.x = ld_at<float>(xb, rowoff);
            if constexpr (MASK) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    w.mf[k] = 0.f;
                    w.mb[k] = 0;
                    if (p.mask_kind[k] == 2) w.mf[k] = ld_at<float>(mfp[k], rowoff);
                    else if (p.mask_kind[k] == 1) w.mb[k] = ld_at<uint8_t>(mbp[k], rowoff);
                }
            }
            if constexpr (BCF) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    w.bf[k] = 0.f;
                    if (p.bcf[k]) w.bf[k] = ld_at<float>(bcfb[k], rowoff);
                }
            }
            if constexpr (FGP) {
                const unsigned eoff = (unsigned)min(max(r - 1, 0), p.nely - 1) * (unsigned)p.nelx + L.qe;
#pragma unroll
                for (int g = 0; g < G; ++g) w.f[g] = ld_at<float>(fg, eoff + (unsigned)(g * L.nel));
            }
        };

        // the two Dirichlet substitutions of a landed row (condition 2 wins on u; the cotangent of a Dirichlet row is zero) and the
        // right neighbours
        auto consume = [&](const Raw& w, Row& R) {
            float val = 0.f, lv = 0.f;
            if constexpr (NEEDU) val = w.v;
            if constexpr (VJP) lv = w.x * lscale;
            R.fixed = false;
            R.bv = 0.f;
            if constexpr (MASK) {
                bool fx[2];
                float bv[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    fx[k] = p.mask_kind[k] == 2 ? (w.mf[k] >= 0.5f) : (p.mask_kind[k] == 1 ? (w.mb[k] != 0) : false);
                    bv[k] = p.bcv[k];
                    if constexpr (BCF) bv[k] = p.bcf[k] ? w.bf[k] : bv[k];
                }
                R.fixed = fx[0] || fx[1];
                val = fx[1] ? bv[1] : (fx[0] ? bv[0] : val);
                const bool first = fx[0] && (p.r_first_wins != 0 || !fx[1]);
                R.bv = first ? bv[0] : bv[1];
                lv = R.fixed ? 0.f : lv;
            }
            if constexpr (NEEDU) {
                R.c = val;
                R.n = __shfl_down(val, 1, 64);
            }
            if constexpr (NU) {
                R.nuc = w.nu;
                R.nun = __shfl_down(w.nu, 1, 64);
            }
            if constexpr (VJP) {
                R.lc = lv;
                R.ln = __shfl_down(lv, 1, 64);
            }
        };

        // the lane's element in element row e (node rows e, e + 1: Bm, Tp): its four local contributions, zero where the element does
        // not exist; returns the parts that belong to the lane's node in rows e (bot) and e + 1 (top)
        auto element = [&](const Row& Bm, const Row& Tp, const Raw& w, int e, float (&bot)[1], float (&top)[1]) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int jg = 0; jg < NGP; ++jg) {
                const float by0 = p.tb.by[jg][0], by1 = p.tb.by[jg][1], dy0 = p.tb.dy[jg][0], dy1 = p.tb.dy[jg][1];
#pragma unroll
                for (int ig = 0; ig < NGP; ++ig) {
                    const int g = jg * NGP + ig;
                    const float bx0 = p.tb.bx[ig][0], bx1 = p.tb.bx[ig][1], dx0 = p.tb.dx[ig][0], dx1 = p.tb.dx[ig][1];
                    float ug = 0.f, ux = 0.f, uy = 0.f;
                    if constexpr (NEEDU) q1_eval(bx0, bx1, dx0, dx1, by0, by1, dy0, dy1, Bm.c, Bm.n, Tp.c, Tp.n, ug, ux, uy);
                    float kxn = p.kx, kyn = p.ky;
                    if constexpr (NU) {
                        const float nug = fmaf(by0, fmaf(bx0, Bm.nuc, bx1 * Bm.nun), by1 * fmaf(bx0, Tp.nuc, bx1 * Tp.nun));
                        kxn *= nug;
                        kyn *= nug;
                    }
                    float A, Bc, Cc;
                    if constexpr (VJP) {
                        float L, Lx, Ly;
                        q1_eval(bx0, bx1, dx0, dx1, by0, by1, dy0, dy1, Bm.lc, Bm.ln, Tp.lc, Tp.ln, L, Lx, Ly);
                        const float qq = fmaf(p.tax, Lx, fmaf(p.tay, Ly, L));
                        A = 0.f;
                        if constexpr (REACT) A = L * fmaf(fmaf(3.f * p.c3, ug, 2.f * p.c2), ug, p.c1);
                        Bc = fmaf(p.ax, qq, kxn * Lx);
                        Cc = fmaf(p.ay, qq, kyn * Ly);
                    } else {
                        float f = p.fconst;
                        if constexpr (FGP) f = w.f[g];
                        const float s = fmaf(p.ax, ux, p.ay * uy) - f;
                        A = s + p.c0;
                        if constexpr (REACT) A = s + fmaf(fmaf(fmaf(p.c3, ug, p.c2), ug, p.c1), ug, p.c0);
                        Bc = fmaf(kxn, ux, p.tax * s);
                        Cc = fmaf(kyn, uy, p.tay * s);
                    }
                    q1_flux_scatter(bx0, bx1, dx0, dx1, by0, by1, dy0, dy1, p.tb.wg[g], A, Bc, Cc, acc);
                }
            }
            q1_owner_handover(L.elem_x && e >= 0 && e < p.nely, acc, bot[0], top[0]);
        };

        // node row e of the residual
        auto finish = [&](int e, const Row& R, const float (&carry)[1], const float (&bot)[1]) {
            const unsigned rowoff = (unsigned)e * (unsigned)nx + L.qc;
            float r = carry[0] + bot[0];
            // forward: Dirichlet rows take the boundary value (the scripts' torch.where); VJP: no gradient reaches a substituted node
            if constexpr (MASK) r = R.fixed ? (VJP ? 0.f : R.bv) : r;
            sq[0] = L.owner ? fmaf(r, r, sq[0]) : sq[0];
            if (L.owner && ob) st_at<float>(ob, rowoff, r);
        };

        const int j0 = strip * p.rows_per_strip, j1 = min(j0 + p.rows_per_strip, ny);
        constexpr int NF = 1;
#include "q1_owner_march.inl"
    }
    if (p.want_sums) finish_sums<1>(p.part, p.counter, p.sumsq, p.norm, sq, (int)threadIdx.x, (int)blockDim.x, red, &last_flag);
}

#define TR_LAUNCH(...) hipLaunchKernelGGL((transport2d_kernel<__VA_ARGS__>), grid, block, 0, s, pp)

// MASK / BCF: 0 none, 1 conditions with constants, 2 with a value field
template <int NGP, bool NU, bool FGP, bool REACT, bool VJP>
static void transport_launch_mask(const TransportParams& pp, int sel, dim3 grid, dim3 block, hipStream_t s) {
    constexpr bool NEEDU = !VJP || REACT;
    if constexpr (NEEDU) {
        if (sel == 2) { TR_LAUNCH(NGP, true, true, NU, FGP, REACT, VJP); return; }
    }
    if (sel >= 1) TR_LAUNCH(NGP, true, false, NU, FGP, REACT, VJP);
    else TR_LAUNCH(NGP, false, false, NU, FGP, REACT, VJP);
}

template <int NGP, bool NU, bool REACT>
static void transport_launch_mode(const TransportParams& pp, int sel, bool vjp, dim3 grid, dim3 block, hipStream_t s) {
    if (vjp) transport_launch_mask<NGP, NU, false, REACT, true>(pp, sel, grid, block, s);       // the VJP does not read the forcing
    else if (pp.fgp) transport_launch_mask<NGP, NU, true, REACT, false>(pp, sel, grid, block, s);
    else transport_launch_mask<NGP, NU, false, REACT, false>(pp, sel, grid, block, s);
}

template <int NGP>
static void transport_launch_ngp(const TransportParams& pp, int sel, bool react, bool vjp, dim3 grid, dim3 block, hipStream_t s) {
    if (pp.nu) {
        if (react) transport_launch_mode<NGP, true, true>(pp, sel, vjp, grid, block, s);
        else transport_launch_mode<NGP, true, false>(pp, sel, vjp, grid, block, s);
    } else {
        if (react) transport_launch_mode<NGP, false, true>(pp, sel, vjp, grid, block, s);
        else transport_launch_mode<NGP, false, false>(pp, sel, vjp, grid, block, s);
    }
}

constexpr int TRANSPORT_MIN_ROWS = 8;          // shortest strip (flow2d_plan): a strip recomputes one halo element row

static inline int64_t transport_workspace_bytes(const Flow2dGeom& g, int batch) {
    return DN_WS_HEADER + (int64_t)sizeof(double) * g.gx * batch;
}

}  // namespace dn

using namespace dn;

extern "C" int64_t dn_transport_workspace_bytes(const dn_mesh* m) {
    if (flow2d_validate(m) != 0) return DN_E_BADARG;
    return transport_workspace_bytes(flow2d_plan(m, TRANSPORT_MIN_ROWS), m->batch);
}

extern "C" int dn_transport_apply(const dn_mesh* m, const dn_transport_args* a, void* stream) {
    int rc = flow2d_validate(m);
    if (rc) return rc;
    if (!a || !a->u) return DN_E_BADARG;
    if (!a->out && !a->sumsq && !a->norm) return DN_E_BADARG;
    if (a->in_den && !a->in_num) return DN_E_BADARG;
    if ((a->vjp | a->r_first_wins | a->nu_batched | a->f_batched) & ~1) return DN_E_BADARG;
    for (int k = 0; k < 2; ++k) {
        if ((a->mask_is_u8[k] | a->mask_batched[k] | a->bc_field_batched[k]) & ~1) return DN_E_BADARG;
        if (a->bc_field[k] && !a->bc_mask[k]) return DN_E_BADARG;           // a value field without a condition
    }
    const bool vjp = a->vjp != 0;
    if (vjp && !a->cot) return DN_E_BADARG;                                  // a VJP without its cotangent
    if (!vjp && a->in_num) return DN_E_BADARG;                               // the scaling applies to the cotangent only
    const Flow2dGeom g = flow2d_plan(m, TRANSPORT_MIN_ROWS);
    const bool want_red = a->sumsq || a->norm;
    if (want_red && (!a->workspace || a->workspace_bytes < transport_workspace_bytes(g, m->batch))) return DN_E_WORKSPACE;

    TransportParams pp;
    const int ngp = m->ngp;
    q1_tables_fill(pp.tb, m, a->wscale);
    const bool react = a->react[1] != 0.f || a->react[2] != 0.f || a->react[3] != 0.f;
    const bool needu = !vjp || react;
    pp.u = a->u;
    pp.nu = a->nu;
    pp.nu_batched = a->nu_batched;
    bool mask = false, bcf = false;
    for (int k = 0; k < 2; ++k) {
        pp.mask[k] = a->bc_mask[k];
        pp.mask_kind[k] = !a->bc_mask[k] ? 0 : (a->mask_is_u8[k] ? 1 : 2);
        pp.mask_batched[k] = a->mask_batched[k];
        pp.bcf[k] = needu ? a->bc_field[k] : nullptr;
        pp.bcf_batched[k] = a->bc_field_batched[k];
        pp.bcv[k] = a->bc_value[k];
        mask = mask || a->bc_mask[k];
        bcf = bcf || pp.bcf[k];
    }
    pp.r_first_wins = a->r_first_wins;
    pp.fgp = vjp ? nullptr : a->f_gp;
    pp.fgp_batched = a->f_batched;
    pp.fconst = a->f_gp ? 0.f : a->f_value;
    pp.cot = vjp ? a->cot : nullptr;
    pp.in_num = a->in_num;
    pp.in_den = a->in_den;
    pp.out = a->out;
    pp.counter = reinterpret_cast<unsigned*>(a->workspace);
    pp.part = a->workspace ? reinterpret_cast<double*>(reinterpret_cast<char*>(a->workspace) + DN_WS_HEADER) : nullptr;
    pp.sumsq = a->sumsq;
    pp.norm = a->norm;
    pp.ax = a->adv[0]; pp.ay = a->adv[1];
    pp.kx = a->kappa[0]; pp.ky = a->kappa[1];
    pp.tax = a->tau * a->adv[0]; pp.tay = a->tau * a->adv[1];
    pp.c0 = a->react[0]; pp.c1 = a->react[1]; pp.c2 = a->react[2]; pp.c3 = a->react[3];
    pp.nx = m->nx; pp.ny = m->ny;
    pp.nelx = m->nx - 1; pp.nely = m->ny - 1;
    pp.chunks = g.chunks; pp.rows_per_strip = g.R; pp.strips = g.strips;
    pp.want_sums = want_red ? 1 : 0;

    const dim3 grid(g.gx, m->batch), block(64 * g.wpb);
    const int sel = mask ? (bcf ? 2 : 1) : 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (ngp) {
        case 2: transport_launch_ngp<2>(pp, sel, react, vjp, grid, block, s); break;
        case 3: transport_launch_ngp<3>(pp, sel, react, vjp, grid, block, s); break;
        default: transport_launch_ngp<4>(pp, sel, react, vjp, grid, block, s); break;
    }
    DN_LAUNCH_CHECK();
    return 0;
}
