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
#include <algorithm>

#include "fsdt_common.h"

namespace dn {

struct StokesParams {
    float mx[2][2], kx[2][2], cx[2][2];    // 1-D element matrices along x (derivatives scaled by 2 / hx)
    float my[2][2], ky[2][2], cy[2][2];    // along y, times wscale
    float lx[2], ly[2];                    // sum_g w_g N_a (ly times wscale): constant forcing
    float fw[4][16];                       // Gauss-point forcing weights: wscale w_ig w_jg N_lx(ig) N_ly(jg); local node ly * 2 + lx, point jg * ngp + ig
    float visco, pspg, sgn3;               // sgn3: -1 in the transpose launch
    float fconst[2];                       // constant forcing (where fgp[k] is NULL)
    const float* fld[3];                   // u, v, p
    const void* mask[3];
    int mask_kind[3];                      // 0: none, 1: uint8 (!= 0), 2: fp32 (>= 0.5)
    int mask_batched[3];
    const float* bcf[3];
    int bcf_batched[3];
    float bcv[3];
    const float* fgp[2];                   // (B | 1, G, nely, nelx)
    int fgp_batched[2];
    const float* in_num;                   // optional 3 + 3 device floats: field k is scaled by in_num[k] / in_den[k] (0 where in_den[k] <= 0)
    const float* in_den;
    float* out[3];
    double* part;                          // [3][nblocks] partial sums of squares (finish_sums3)
    unsigned* counter;
    double* sumsq;
    float* norms;
    int nx, ny, nelx, nely, chunks, rows_per_strip, strips, want_sums;
};

constexpr int STOKES_OWNERS = 62;          // owner lanes per wave (lanes 1 .. 62); lanes 0 and 63 are ghosts

// Raw loads of one node row r (clamped into the mesh) and, with the Gauss-point forcing, of the element layer r - 1 under it
template <int G, bool MASK, bool BCF, bool FGP>
struct StokesRaw {
    float v[3];
    float mf[MASK ? 3 : 1];
    uint8_t mb[MASK ? 3 : 1];
    float bf[BCF ? 3 : 1];
    float f[FGP ? 2 : 1][FGP ? G : 1];
};

template <int NGP, bool MASK, bool BCF, bool FGP>
__global__ void __launch_bounds__(256) stokes2d_kernel(const StokesParams p) {
    constexpr int G = NGP * NGP;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = (int)threadIdx.x & 63;
    const int wid = (int)blockIdx.x * ((int)blockDim.x >> 6) + wave;
    const int b = blockIdx.y;
    const int chunk = wid % p.chunks, strip = wid / p.chunks;

    __shared__ double red[16];
    __shared__ int last_flag;
    float sq[3] = {0.f, 0.f, 0.f};

    if (strip < p.strips) {
        const int nx = p.nx, ny = p.ny;
        const int q = chunk * STOKES_OWNERS + lane - 1;                    // node column of the lane
        const bool owner = lane >= 1 && lane <= STOKES_OWNERS && q < nx;
        const unsigned qc = (unsigned)min(max(q, 0), nx - 1);
        const float lf = q > 0 ? 1.f : 0.f, rf = q < nx - 1 ? 1.f : 0.f;   // element to the left / right of the node exists
        const int64_t nps = (int64_t)nx * ny;
        const int nel = p.nelx * p.nely;

        const float* fb[3];
        const float* bcf[3];
        const float* mfp[3];
        const uint8_t* mbp[3];
        float* ob[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            fb[k] = p.fld[k] + (int64_t)b * nps;
            bcf[k] = p.bcf[k] ? p.bcf[k] + (p.bcf_batched[k] ? (int64_t)b * nps : 0) : fb[k];
            const int64_t mo = p.mask_batched[k] ? (int64_t)b * nps : 0;
            mfp[k] = reinterpret_cast<const float*>(p.mask[k]) + (p.mask_kind[k] == 2 ? mo : 0);
            mbp[k] = reinterpret_cast<const uint8_t*>(p.mask[k]) + (p.mask_kind[k] == 1 ? mo : 0);
            ob[k] = p.out[k] ? p.out[k] + (int64_t)b * nps : nullptr;
        }
        const float* fg[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) fg[k] = p.fgp[k] ? p.fgp[k] + (p.fgp_batched[k] ? (int64_t)b * G * nel : 0) : nullptr;

        float fscale[3] = {1.f, 1.f, 1.f};
        if (p.in_num) {               // cotangent of the norms over the norms (the VJP of ||R_k||), torch's convention at ||R_k|| == 0: zero
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float den = p.in_den[k];
                fscale[k] = den > 0.f ? p.in_num[k] / den : (den == den ? 0.f : den);
            }
        }
        fscale[2] *= p.sgn3;

        // per-lane coefficients (left, centre, right neighbour) of the assembled 1-D x operators: the left element's row 1, the right element's row 0
        const float kL = lf * p.kx[1][0], kC = lf * p.kx[1][1] + rf * p.kx[0][0], kR = rf * p.kx[0][1];
        const float mL = lf * p.mx[1][0], mC = lf * p.mx[1][1] + rf * p.mx[0][0], mR = rf * p.mx[0][1];
        const float cL = lf * p.cx[1][0], cC = lf * p.cx[1][1] + rf * p.cx[0][0], cR = rf * p.cx[0][1];
        const float tL = lf * p.cx[0][1], tC = lf * p.cx[1][1] + rf * p.cx[0][0], tR = rf * p.cx[1][0];      // C^T
        const float lxa = lf * p.lx[1] + rf * p.lx[0];
        const bool elem_x = q >= 0 && q < p.nelx;                           // the element to the right of the lane's column
        const unsigned qe = (unsigned)min(max(q, 0), p.nelx - 1);

        using Raw = StokesRaw<G, MASK, BCF, FGP>;
        auto issue = [&](int r, Raw& w) {
            const unsigned rowoff = (unsigned)min(max(r, 0), ny - 1) * (unsigned)nx + qc;
#pragma unroll
            for (int k = 0; k < 3; ++k) w.v[k] = ld_at<float>(fb[k], rowoff);
            if constexpr (MASK) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    w.mf[k] = 0.f;
                    w.mb[k] = 0;
                    if (p.mask_kind[k] == 2) w.mf[k] = ld_at<float>(mfp[k], rowoff);
                    else if (p.mask_kind[k] == 1) w.mb[k] = ld_at<uint8_t>(mbp[k], rowoff);
                }
            }
            if constexpr (BCF) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    w.bf[k] = 0.f;
                    if (p.bcf[k]) w.bf[k] = ld_at<float>(bcf[k], rowoff);
                }
            }
            if constexpr (FGP) {
                const unsigned eoff = (unsigned)min(max(r - 1, 0), p.nely - 1) * (unsigned)p.nelx + qe;
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int g = 0; g < G; ++g) w.f[k][g] = fg[k] ? ld_at<float>(fg[k], eoff + (unsigned)(g * nel)) : 0.f;
            }
        };

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
                    const bool fx = p.mask_kind[k] == 2 ? (w.mf[k] >= 0.5f) : (p.mask_kind[k] == 1 ? (w.mb[k] != 0) : false);
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
                const float ok = (elem_x && e >= 0 && e < p.nely) ? 1.f : 0.f;
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
                    // the node's own element (right) as local node lx = 0, the left neighbour's element as lx = 1
                    bot[k] = c[0] + __shfl_up(c[1], 1, 64);
                    top[k] = c[2] + __shfl_up(c[3], 1, 64);
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
            const unsigned rowoff = (unsigned)j * (unsigned)nx + qc;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float r = R[k];
                if constexpr (MASK) r = (fixc & (1u << k)) ? bvc[k] : r;      // Dirichlet rows take the boundary value (the scripts' torch.where)
                sq[k] = owner ? fmaf(r, r, sq[k]) : sq[k];
                if (owner && ob[k]) st_at<float>(ob[k], rowoff, r);
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
    if (p.want_sums) finish_sums3(p, sq, (int)threadIdx.x, (int)blockDim.x, red, &last_flag);
}

static constexpr int64_t STOKES_WS_HEADER = 64 * (1 + 64);     // top counter + DN_NSHARD shard counters (finish_sums3)

struct StokesGeom { int chunks, strips, R, wpb, gx; };

static int stokes_validate(const dn_mesh* m) {
    if (!m) return DN_E_BADARG;
    if (m->nsd != 2 || m->degree != 1 || m->ngp < 2 || m->ngp > 4) return DN_E_UNSUPPORTED;
    if (m->batch < 1 || m->batch > 65535 || m->nx < 2 || m->ny < 2) return DN_E_BADARG;
    const int64_t nps = (int64_t)m->nx * m->ny, nel = (int64_t)(m->nx - 1) * (m->ny - 1);
    if (nps >= (1ll << 30) || nel * m->ngp * m->ngp >= (1ll << 30)) return DN_E_UNSUPPORTED;     // 32-bit byte offsets within a sample
    return 0;
}

// One wave per (62-column chunk, strip of R node rows, sample); strips as short as 4 rows until the launch has ~4096 waves (16 per CU:
// the kernel streams its rows from HBM, and the latency of a row's loads is hidden by the other waves of the SIMD and the one-row prefetch).
// A strip re-reads one node row above and below it.
static StokesGeom stokes_plan(const dn_mesh* m) {
    StokesGeom g;
    g.chunks = (m->nx + STOKES_OWNERS - 1) / STOKES_OWNERS;
    const int64_t per_row = (int64_t)g.chunks * m->batch;
    int strips = (int)std::min<int64_t>((4096 + per_row - 1) / per_row, (m->ny + 3) / 4);
    strips = std::max(strips, 1);
    g.R = (m->ny + strips - 1) / strips;
    g.strips = (m->ny + g.R - 1) / g.R;
    const int waves = g.chunks * g.strips;
    g.wpb = std::min(waves, 4);
    g.gx = (waves + g.wpb - 1) / g.wpb;
    return g;
}

template <int NGP>
static void stokes_launch_k(const StokesParams& pp, const StokesGeom& g, int batch, bool mask, bool bcf, bool fgp, hipStream_t s) {
    dim3 grid(g.gx, batch), block(64 * g.wpb);
    const int sel = (mask ? (bcf ? 2 : 1) : 0);
    if (fgp) {
        switch (sel) {
            case 0: hipLaunchKernelGGL((stokes2d_kernel<NGP, false, false, true>), grid, block, 0, s, pp); return;
            case 1: hipLaunchKernelGGL((stokes2d_kernel<NGP, true, false, true>), grid, block, 0, s, pp); return;
            default: hipLaunchKernelGGL((stokes2d_kernel<NGP, true, true, true>), grid, block, 0, s, pp); return;
        }
    }
    switch (sel) {      // without Gauss-point forcing the rule only enters the matrices: one instantiation serves every rule
        case 0: hipLaunchKernelGGL((stokes2d_kernel<2, false, false, false>), grid, block, 0, s, pp); return;
        case 1: hipLaunchKernelGGL((stokes2d_kernel<2, true, false, false>), grid, block, 0, s, pp); return;
        default: hipLaunchKernelGGL((stokes2d_kernel<2, true, true, false>), grid, block, 0, s, pp); return;
    }
}

}  // namespace dn

using namespace dn;

extern "C" int64_t dn_stokes_workspace_bytes(const dn_mesh* m) {
    if (stokes_validate(m) != 0) return DN_E_BADARG;
    const StokesGeom g = stokes_plan(m);
    return STOKES_WS_HEADER + (int64_t)(3 * sizeof(double)) * g.gx * m->batch;
}

extern "C" int dn_stokes_apply(const dn_mesh* m, const dn_stokes_args* a, void* stream) {
    int rc = stokes_validate(m);
    if (rc) return rc;
    if (!a || !a->u || !a->v || !a->p) return DN_E_BADARG;
    if (!a->out[0] && !a->out[1] && !a->out[2] && !a->sumsq && !a->norms) return DN_E_BADARG;
    if ((a->in_num != nullptr) != (a->in_den != nullptr)) return DN_E_BADARG;
    for (int k = 0; k < 3; ++k) {
        if ((a->mask_is_u8[k] | a->mask_batched[k] | a->bc_field_batched[k]) & ~1) return DN_E_BADARG;
        if (a->bc_field[k] && !a->bc_mask[k]) return DN_E_BADARG;           // a value field without a condition
    }
    for (int k = 0; k < 2; ++k)
        if (a->f_batched[k] & ~1) return DN_E_BADARG;
    const bool want_red = a->sumsq || a->norms;
    const StokesGeom g = stokes_plan(m);
    const int64_t nwg = (int64_t)g.gx * m->batch;
    if (want_red && (!a->workspace || a->workspace_bytes < STOKES_WS_HEADER + (int64_t)(3 * sizeof(double)) * nwg)) return DN_E_WORKSPACE;

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
    pp.fld[0] = a->u; pp.fld[1] = a->v; pp.fld[2] = a->p;
    bool any_mask = false, any_bcf = false;
    for (int k = 0; k < 3; ++k) {
        pp.mask[k] = a->bc_mask[k];
        pp.mask_kind[k] = !a->bc_mask[k] ? 0 : (a->mask_is_u8[k] ? 1 : 2);
        pp.mask_batched[k] = a->mask_batched[k];
        any_mask = any_mask || a->bc_mask[k];
        // the transpose launch: zero Dirichlet values (the projector onto the free nodes)
        pp.bcf[k] = tr ? nullptr : a->bc_field[k];
        pp.bcf_batched[k] = a->bc_field_batched[k];
        pp.bcv[k] = tr ? 0.f : a->bc_value[k];
        any_bcf = any_bcf || pp.bcf[k];
        pp.out[k] = a->out[k];
    }
    bool any_fgp = false;
    for (int k = 0; k < 2; ++k) {
        pp.fgp[k] = tr ? nullptr : a->f_gp[k];
        pp.fgp_batched[k] = a->f_batched[k];
        pp.fconst[k] = (tr || a->f_gp[k]) ? 0.f : a->f_value[k];
        any_fgp = any_fgp || pp.fgp[k];
    }
    pp.in_num = a->in_num;
    pp.in_den = a->in_den;
    pp.counter = reinterpret_cast<unsigned*>(a->workspace);
    pp.part = a->workspace ? reinterpret_cast<double*>(reinterpret_cast<char*>(a->workspace) + STOKES_WS_HEADER) : nullptr;
    pp.sumsq = a->sumsq;
    pp.norms = a->norms;
    pp.nx = m->nx; pp.ny = m->ny;
    pp.nelx = m->nx - 1; pp.nely = m->ny - 1;
    pp.chunks = g.chunks; pp.rows_per_strip = g.R; pp.strips = g.strips;
    pp.want_sums = want_red ? 1 : 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (ngp) {
        case 2: stokes_launch_k<2>(pp, g, m->batch, any_mask, any_bcf, any_fgp, s); break;
        case 3: stokes_launch_k<3>(pp, g, m->batch, any_mask, any_bcf, any_fgp, s); break;
        default: stokes_launch_k<4>(pp, g, m->batch, any_mask, any_bcf, any_fgp, s); break;
    }
    DN_LAUNCH_CHECK();
    return 0;
}
