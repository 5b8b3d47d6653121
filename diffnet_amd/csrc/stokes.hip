// Fused 2-D Stokes (PSPG) residuals on Q1 meshes: dn_stokes_apply (include/diffnet_hip.h).
//
// The residual body of examples/stokes/single_instance/e2_stokes_ldc_resmin.py:151-240 of the reference (and of its siblings listed in the
// header): Dirichlet substitution of u, v, p, nine Gauss-point evaluations, the three weak forms
//     R1_a = sum_e sum_g J w_g [ nu (Nx_a u_x + Ny_a u_y) - Nx_a p - N_a f1 ]
//     R2_a = sum_e sum_g J w_g [ nu (Nx_a v_x + Ny_a v_y) - Ny_a p - N_a f2 ]
//     R3_a = sum_e sum_g J w_g [ N_a (u_x + v_y) + tau (Nx_a p_x + Ny_a p_y) ]
// their assembly, the Dirichlet rows (which take the boundary VALUE) and the three sums of squares -- in one launch.
//
// Factorisation: nu, tau and J are constants and the mesh is uniform, so every operator term is a tensor product of two assembled 1-D
// operators built from the 2 x 2 element matrices of the quadrature rule (exact for any rule; formed on the host in double precision from
// the mesh's own tables):
//     M[a][b] = sum_g w_g N_a N_b     K[a][b] = sum_g w_g N_a' N_b'     C[a][b] = sum_g w_g N_a' N_b     (C^T: test value, trial derivative)
//     R1 = nu (K_x (x) M_y + M_x (x) K_y) u - (C_x (x) M_y) p - F1
//     R2 = nu (K_x (x) M_y + M_x (x) K_y) v - (M_x (x) C_y) p - F2
//     R3 = (C_x^T (x) M_y) u + (M_x (x) C_y^T) v + tau (K_x (x) M_y + M_x (x) K_y) p
// Assembled along a node row, a 1-D operator is a 3-point stencil whose end points only take the element that exists (the factors lf / rf
// below), so the boundary-node stencils come out of the same code.  The Gauss-point forcing is not a tensor product (it varies per element):
// each lane reduces the forcing of the element to its right against the four local basis functions and hands the two right-hand values to
// its neighbour (shuffle); the top pair is carried to the next node row.
//
// Node-owner march: one wave = 62 owner columns + two ghost lanes that only supply the x halo; a lane marches the node rows of a strip
// keeping the x-factor products of three rows (8 per row) in registers; x neighbours come over ds_bpermute (__shfl_up / __shfl_down).
// Every output node is written once by its owner; no atomics on the data path; sums of squares: fixed-order fp64 reduction (finish_sums3).
//
// Adjoint: J_R = P A P with A's coupling blocks -C (momentum) and C^T (continuity), so J_R^T = S J_R S with S = diag(1, 1, -1).  The
// transpose launch is this kernel with p negated as it is loaded, R3 negated before its Dirichlet rows, no forcing and zero Dirichlet values.
#include "flow2d_common.h"      // everything the kernel shares with navier_stokes.hip: parameters, lane set-up, row loader, plan, checks, launch switch

namespace dn {

struct StokesParams : Flow2dParams {
    float mx[2][2], kx[2][2], cx[2][2];    // 1-D element matrices along x (derivatives scaled by 2 / hx)
    float my[2][2], ky[2][2], cy[2][2];    // along y, times wscale
    float lx[2], ly[2];                    // sum_g w_g N_a (ly times wscale): constant forcing
    float fw[4][16];                       // Gauss-point forcing weights: wscale w_ig w_jg N_lx(ig) N_ly(jg); local node ly * 2 + lx, point jg * ngp + ig
    float visco, pspg, sgn3;               // sgn3: -1 in the transpose launch
};

template <int NGP, bool MASK, bool BCF, bool FGP>
__global__ void __launch_bounds__(256) stokes2d_kernel(const StokesParams p) {
    constexpr int G = NGP * NGP;
    int lane, chunk, strip;
    flow2d_wave(p, lane, chunk, strip);

    __shared__ double red[16];
    __shared__ int last_flag;
    float sq[3] = {0.f, 0.f, 0.f};

    if (strip < p.strips) {
        const int nx = p.nx, ny = p.ny;
        Flow2dLane<0> L;
        flow2d_lane(p, chunk, lane, L);
        const int q = L.q;
        const float lf = q > 0 ? 1.f : 0.f, rf = q < nx - 1 ? 1.f : 0.f;   // element to the left / right of the node exists
#pragma unroll
        for (int k = 0; k < 3; ++k) flow2d_field_base<G>(p, (int)blockIdx.y, k, L);

        float fscale[3];               // in_num / in_den scales the fields
        flow2d_in_scale(p, fscale);
        fscale[2] *= p.sgn3;

        // per-lane coefficients (left, centre, right neighbour) of the assembled 1-D x operators: the left element's row 1, the right element's row 0
        const float kL = lf * p.kx[1][0], kC = lf * p.kx[1][1] + rf * p.kx[0][0], kR = rf * p.kx[0][1];
        const float mL = lf * p.mx[1][0], mC = lf * p.mx[1][1] + rf * p.mx[0][0], mR = rf * p.mx[0][1];
        const float cL = lf * p.cx[1][0], cC = lf * p.cx[1][1] + rf * p.cx[0][0], cR = rf * p.cx[0][1];
        const float tL = lf * p.cx[0][1], tC = lf * p.cx[1][1] + rf * p.cx[0][0], tR = rf * p.cx[1][0];      // C^T
        const float lxa = lf * p.lx[1] + rf * p.lx[0];

        using Raw = Flow2dRaw<G, MASK, BCF, FGP, 0>;
        auto issue = [&](int r, Raw& w) { flow2d_issue(p, L, r, w); };

        // a landed row: scaling, Dirichlet substitution, the x-factor products X[0..7]
        //   0: nu K u - C p   1: nu M u   2: nu K v   3: nu M v   4: -M p   5: C^T u + tau K p   6: M v   7: tau M p
        auto consume = [&](const Raw& w, float (&X)[8], unsigned& fixed, float (&bv)[3]) {
            float c[3];
            fixed = 0u;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float val = w.v[k] * fscale[k];
                bv[k] = p.bcv[k];
                if constexpr (MASK) {
                    const bool fx = flow2d_fixed(p, w, k);
                    if constexpr (BCF) bv[k] = p.bcf[k] ? w.bf[k] : bv[k];
                    val = fx ? bv[k] : val;
                    fixed |= fx ? (1u << k) : 0u;
                }
                c[k] = val;
            }
            float l[3], r[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                l[k] = __shfl_up(c[k], 1, 64);
                r[k] = __shfl_down(c[k], 1, 64);
            }
            const float Ku = fmaf(kL, l[0], fmaf(kC, c[0], kR * r[0]));
            const float Mu = fmaf(mL, l[0], fmaf(mC, c[0], mR * r[0]));
            const float Tu = fmaf(tL, l[0], fmaf(tC, c[0], tR * r[0]));
            const float Kv = fmaf(kL, l[1], fmaf(kC, c[1], kR * r[1]));
            const float Mv = fmaf(mL, l[1], fmaf(mC, c[1], mR * r[1]));
            const float Kp = fmaf(kL, l[2], fmaf(kC, c[2], kR * r[2]));
            const float Mp = fmaf(mL, l[2], fmaf(mC, c[2], mR * r[2]));
            const float Cp = fmaf(cL, l[2], fmaf(cC, c[2], cR * r[2]));
            X[0] = fmaf(p.visco, Ku, -Cp);
            X[1] = p.visco * Mu;
            X[2] = p.visco * Kv;
            X[3] = p.visco * Mv;
            X[4] = -Mp;
            X[5] = fmaf(p.pspg, Kp, Tu);
            X[6] = Mv;
            X[7] = p.pspg * Mp;
        };
        // the forcing of the element layer a landed row carries: (bottom, top) contributions to the lane's node of the rows below / above it
        auto layer_forcing = [&](const Raw& w, int e, float (&bot)[2], float (&top)[2]) {
            if constexpr (FGP) {
                const float ok = (L.elem_x && e >= 0 && e < p.nely) ? 1.f : 0.f;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    float c[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        float s = 0.f;
#pragma unroll
                        for (int g = 0; g < G; ++g) s = fmaf(p.fw[a][g], w.f[k][g], s);
                        c[a] = ok * s;
                    }
                    q1_owner_handover(c, bot[k], top[k]);
                }
            } else {
                bot[0] = bot[1] = top[0] = top[1] = 0.f;
            }
        };

        const int j0 = strip * p.rows_per_strip, j1 = min(j0 + p.rows_per_strip, ny);
        float Xm[8], Xc[8], Xp[8];
        unsigned fixc, fixp, fix_unused;
        float bvc[3], bvp[3], bv_unused[3];
        float carry[2];
        // two rows in flight ahead of the one being finished (W0, W1 alternate; the loop is unrolled by two so that no register with a load
        // outstanding is ever copied -- a copy would wait for it)
        Raw W0, W1;
        {
            Raw A, Bw;
            issue(j0 - 1, A);
            issue(j0, Bw);
            issue(j0 + 1, W0);
            issue(j0 + 2, W1);
            consume(A, Xm, fix_unused, bv_unused);
            consume(Bw, Xc, fixc, bvc);
            float bot[2];
            layer_forcing(Bw, j0 - 1, bot, carry);
        }
        // node row j: W holds the raw row j + 1 (and the element layer j); refilled with row j + 3
        auto step = [&](int j, Raw& W) {
            consume(W, Xp, fixp, bvp);
            float bot[2], top[2];
            layer_forcing(W, j, bot, top);
            issue(j + 3, W);
            const float df = j > 0 ? 1.f : 0.f, uf = j < ny - 1 ? 1.f : 0.f;
            const float yMd = df * p.my[1][0], yMc = df * p.my[1][1] + uf * p.my[0][0], yMu = uf * p.my[0][1];
            const float yKd = df * p.ky[1][0], yKc = df * p.ky[1][1] + uf * p.ky[0][0], yKu = uf * p.ky[0][1];
            const float yCd = df * p.cy[1][0], yCc = df * p.cy[1][1] + uf * p.cy[0][0], yCu = uf * p.cy[0][1];
            const float yTd = df * p.cy[0][1], yTc = df * p.cy[1][1] + uf * p.cy[0][0], yTu = uf * p.cy[1][0];      // C^T
            const float lyl = lxa * (df * p.ly[1] + uf * p.ly[0]);
            auto yop = [&](float d, float c, float u, int i) { return fmaf(d, Xm[i], fmaf(c, Xc[i], u * Xp[i])); };
            float R[3];
            R[0] = yop(yMd, yMc, yMu, 0) + yop(yKd, yKc, yKu, 1) - fmaf(p.fconst[0], lyl, carry[0] + bot[0]);
            R[1] = yop(yMd, yMc, yMu, 2) + yop(yKd, yKc, yKu, 3) + yop(yCd, yCc, yCu, 4) - fmaf(p.fconst[1], lyl, carry[1] + bot[1]);
            R[2] = p.sgn3 * (yop(yMd, yMc, yMu, 5) + yop(yTd, yTc, yTu, 6) + yop(yKd, yKc, yKu, 7));
            const unsigned rowoff = (unsigned)j * (unsigned)nx + L.qc;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float r = R[k];
                if constexpr (MASK) r = (fixc & (1u << k)) ? bvc[k] : r;      // Dirichlet rows take the boundary value (the scripts' torch.where)
                sq[k] = L.owner ? fmaf(r, r, sq[k]) : sq[k];
                if (L.owner && L.ob[k]) st_at<float>(L.ob[k], rowoff, r);
            }
            carry[0] = top[0];
            carry[1] = top[1];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                Xm[i] = Xc[i];
                Xc[i] = Xp[i];
            }
            fixc = fixp;
#pragma unroll
            for (int k = 0; k < 3; ++k) bvc[k] = bvp[k];
        };
        for (int j = j0; j < j1; j += 2) {
            step(j, W0);
            if (j + 1 < j1) step(j + 1, W1);
        }
        (void)fix_unused;
    }
    if (p.want_sums) finish_sums3(p.part, p.counter, p.sumsq, p.norms, sq, (int)threadIdx.x, (int)blockDim.x, red, &last_flag);
}

// The kernels of one rule.  Without Gauss-point forcing the rule only enters the matrices: one instantiation serves every rule
template <int NGP>
struct StokesFamily {
    template <bool MASK, bool BCF, bool FGP>
    static void launch(dim3 grid, dim3 block, hipStream_t s, const StokesParams& pp) {
        hipLaunchKernelGGL((stokes2d_kernel<FGP ? NGP : 2, MASK, BCF, FGP>), grid, block, 0, s, pp);
    }
};

constexpr int STOKES_MIN_ROWS = 4;      // shortest strip (flow2d_plan): a strip re-reads one node row above and below it

}  // namespace dn

using namespace dn;

extern "C" int64_t dn_stokes_workspace_bytes(const dn_mesh* m) {
    if (flow2d_validate(m) != 0) return DN_E_BADARG;
    return flow2d_workspace_bytes(flow2d_plan(m, STOKES_MIN_ROWS), m->batch);
}

extern "C" int dn_stokes_apply(const dn_mesh* m, const dn_stokes_args* a, void* stream) {
    int rc = flow2d_validate(m);
    if (rc) return rc;
    if ((rc = flow2d_check_args(a))) return rc;
    const Flow2dGeom g = flow2d_plan(m, STOKES_MIN_ROWS);
    if ((rc = flow2d_check_workspace(a, g, m->batch))) return rc;

    const bool tr = a->transpose != 0;
    StokesParams pp;
    const int ngp = m->ngp;
    const double sx = m->scale[0], sy = m->scale[1], J = a->wscale;
    for (int i = 0; i < 2; ++i) {
        double l = 0.0;
        for (int gq = 0; gq < ngp; ++gq) l += (double)m->gpw[gq] * m->basis[gq][i];
        pp.lx[i] = (float)l;
        pp.ly[i] = (float)(l * J);
        for (int j = 0; j < 2; ++j) {
            double M = 0.0, K = 0.0, Cm = 0.0;
            for (int gq = 0; gq < ngp; ++gq) {
                const double w = m->gpw[gq], ni = m->basis[gq][i], nj = m->basis[gq][j], di = m->dbasis[gq][i], dj = m->dbasis[gq][j];
                M += w * ni * nj;
                K += w * di * dj;
                Cm += w * di * nj;
            }
            pp.mx[i][j] = (float)M;
            pp.kx[i][j] = (float)(K * sx * sx);
            pp.cx[i][j] = (float)(Cm * sx);
            pp.my[i][j] = (float)(M * J);
            pp.ky[i][j] = (float)(K * sy * sy * J);
            pp.cy[i][j] = (float)(Cm * sy * J);
        }
    }
    for (int a4 = 0; a4 < 4; ++a4)
        for (int gq = 0; gq < 16; ++gq) {
            const int lx = a4 & 1, ly = a4 >> 1, ig = gq % ngp, jg = gq / ngp;
            pp.fw[a4][gq] = gq < ngp * ngp ? (float)(J * m->gpw[ig] * m->gpw[jg] * m->basis[ig][lx] * m->basis[jg][ly]) : 0.f;
        }
    pp.visco = a->visco;
    pp.pspg = a->pspg;
    pp.sgn3 = tr ? -1.f : 1.f;
    flow2d_fill(pp, m, a, g);
    if (tr) {       // the transpose launch: zero Dirichlet values (the projector onto the free nodes) and no forcing
        for (int k = 0; k < 3; ++k) {
            pp.bcf[k] = nullptr;
            pp.bcv[k] = 0.f;
        }
        for (int k = 0; k < 2; ++k) {
            pp.fgp[k] = nullptr;
            pp.fconst[k] = 0.f;
        }
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (ngp) {
        case 2: flow2d_launch<StokesFamily<2>>(pp, g, m->batch, s); break;
        case 3: flow2d_launch<StokesFamily<3>>(pp, g, m->batch, s); break;
        default: flow2d_launch<StokesFamily<4>>(pp, g, m->batch, s); break;
    }
    DN_LAUNCH_CHECK();
    return 0;
}
