// Gradient of the Poisson losses with respect to the nodal coefficient nu and the nodal forcing f: dn_poisson_coef_grad
// (include/diffnet_hip.h).
//
// The gradient of the energy with respect to u is linear in (nu, f); this operator is the transpose of that map:
//     g_nu[a] = a_nu in_scale sum_{e contains a} sum_g W_g N_a(g) grad v_g . grad u~_g
//     g_f [a] = a_f  in_scale sum_{e contains a} sum_g W_g N_a(g) v_g                         W_g = gpw_g wscale
// with u~ the field after the two Dirichlet substitutions and v a second nodal field read as ZERO on every Dirichlet node (v absent:
// v = u~, values included).  It replaces what autograd does for the coefficient of the reference's topology optimisation
// (examples/poisson/single_instance/16_topopt.py:119-195).  No reduction, no workspace, no atomics.
//
// 2-D Q1, rules of 2 to 4 points per axis: the element-owner march of q1_owner_march.h with two outputs -- one wave = 62 owner columns +
// two ghost lanes, every node written once, by its owner lane, with the same additions in the same order under any launch plan and any
// batch size: bitwise reproducible.
// Compile-time forms: HASV (v present), WANT (bit 0 g_nu, bit 1 g_f), MK (mask images: none / uint8 / fp32), BCF (a value field).  A call
// with one condition runs the two-condition form with the condition given twice (a substitution is idempotent), and a condition with a
// constant value in a BCF form loads from u and selects the constant: no load sits inside a wave-uniform branch.
//
// 3-D Q1: the plain form.  One thread per node loads the 27 substituted values around it once and adds the contributions of its <= 8
// elements in a fixed order (z, y, x), Gauss point by Gauss point.  Correct and deterministic; unoptimised.
#include <cstdio>

#include "flow2d_common.h"

namespace dn {

enum { CG_MK_NONE = 0, CG_MK_U8 = 1, CG_MK_F32 = 2 };

struct CoefGradParams {
    const float* u;
    const float* v;
    const void* mask[2];
    int mask_batched[2];
    const float* bcf[2];                   // BCF kernels: never NULL (a condition with a constant value points at u)
    int bcf_batched[2];
    int bcf_set[2];
    float bcv[2];
    const float* in_scale;
    float* gnu;
    float* gf;
    float a_nu, a_f;
    Q1Tables tb;                           // wg: 2-D
    float bz[4][2], dz[4][2];              // 3-D: the tables along z
    float w1[4];                           // 3-D: the 1-D weights (wscale rides on a_nu, a_f)
    int nx, ny, nz, nelx, nely, nelz, chunks, rows_per_strip, strips;
};

template <int MK>
struct CgMaskT { using type = uint8_t; };
template <>
struct CgMaskT<CG_MK_F32> { using type = float; };

template <int MK, typename T>
__device__ __forceinline__ bool cg_set(T m) {
    if constexpr (MK == CG_MK_F32) return m > 0.5f;
    else return m != 0;
}

// Raw loads of one node row
template <int MK, bool BCF>
struct CgRaw {
    float u, v;
    typename CgMaskT<MK>::type m[2];
    float bf[BCF ? 2 : 1];
};

// A landed node row: u~ and v of the lane's node (c) and of its right neighbour (n)
struct CgRow {
    float uc = 0.f, un = 0.f, vc = 0.f, vn = 0.f;      // a form sets the ones it reads
};

template <int NGP, bool HASV, int WANT, int MK, bool BCF>
__global__ void __launch_bounds__(256) coef_grad2d_kernel(const CoefGradParams p) {
    constexpr bool WNU = (WANT & 1) != 0, WF = (WANT & 2) != 0;
    constexpr bool NEEDU = WNU || !HASV;            // g_f of a given v does not read u
    constexpr bool MASK = MK != CG_MK_NONE;
    static_assert(MASK || !BCF, "a value field needs its condition");
    static_assert(NEEDU || !BCF, "value fields matter only where u is read");
    using MT = typename CgMaskT<MK>::type;
    int lane, chunk, strip;
    flow2d_wave(p, lane, chunk, strip);
    if (strip >= p.strips) return;

    const int nx = p.nx, ny = p.ny;
    Q1Lane L;
    q1_lane(chunk, lane, nx, p.nelx, p.nely, L);
    const int b = blockIdx.y;
    const int64_t nps = (int64_t)nx * ny;

    const float* ub = p.u + (int64_t)b * nps;
    const float* vb = HASV ? p.v + (int64_t)b * nps : ub;
    float* onu = WNU ? p.gnu + (int64_t)b * nps : nullptr;
    float* of = WF ? p.gf + (int64_t)b * nps : nullptr;
    const MT* mp[2];
    const float* bcfb[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        mp[k] = MASK ? reinterpret_cast<const MT*>(p.mask[k]) + (p.mask_batched[k] ? (int64_t)b * nps : 0) : nullptr;
        bcfb[k] = BCF ? p.bcf[k] + (p.bcf_batched[k] ? (int64_t)b * nps : 0) : ub;
    }
    float sc = 1.f;
    if (p.in_scale) sc = p.in_scale[0];
    const float snu = p.a_nu * sc, sf = p.a_f * sc;

    using Raw = CgRaw<MK, BCF>;
    using Row = CgRow;

    auto issue = [&](int r, Raw& w) {
        const unsigned rowoff = (unsigned)min(max(r, 0), ny - 1) * (unsigned)nx + L.qc;
        if constexpr (NEEDU) w.u = ld_at<float>(ub, rowoff);
        if constexpr (HASV) w.v = ld_at<float>(vb, rowoff);
        if constexpr (MASK) {
#pragma unroll
            for (int k = 0; k < 2; ++k) w.m[k] = ld_at<MT>(mp[k], rowoff);
        }
        if constexpr (BCF) {
#pragma unroll
            for (int k = 0; k < 2; ++k) w.bf[k] = ld_at<float>(bcfb[k], rowoff);
        }
    };

    // the two Dirichlet substitutions of a landed row, in order; v is zero on a Dirichlet node (v absent: v = u~)
    auto consume = [&](const Raw& w, Row& R) {
        float uv = 0.f, vv = 0.f;
        if constexpr (NEEDU) uv = w.u;
        if constexpr (HASV) vv = w.v;
        if constexpr (MASK) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const bool fx = cg_set<MK>(w.m[k]);
                float bv = p.bcv[k];
                if constexpr (BCF) bv = p.bcf_set[k] ? w.bf[k] : bv;
                uv = fx ? bv : uv;
                vv = fx ? 0.f : vv;
            }
        }
        if constexpr (!HASV) vv = uv;
        if constexpr (NEEDU) {
            R.uc = uv;
            R.un = __shfl_down(uv, 1, 64);
        }
        if constexpr (HASV) {
            R.vc = vv;
            R.vn = __shfl_down(vv, 1, 64);
        } else {
            R.vc = R.uc;
            R.vn = R.un;
        }
    };

    // the lane's element in element row e (node rows e, e + 1: Bm, Tp): its four local contributions to each output, zero where the element
    // does not exist; returns the parts that belong to the lane's node in rows e (bot) and e + 1 (top)
    auto element = [&](const Row& Bm, const Row& Tp, const Raw&, int e, float (&bot)[2], float (&top)[2]) {
        float an[4] = {0.f, 0.f, 0.f, 0.f}, af[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jg = 0; jg < NGP; ++jg) {
            const float by0 = p.tb.by[jg][0], by1 = p.tb.by[jg][1], dy1 = p.tb.dy[jg][1];
#pragma unroll
            for (int ig = 0; ig < NGP; ++ig) {
                const float bx0 = p.tb.bx[ig][0], bx1 = p.tb.bx[ig][1], dx1 = p.tb.dx[ig][1];
                const float wq = p.tb.wg[jg * NGP + ig];
                // v at the point and its derivatives.  On a Q1 element N0' = -N1', so a derivative is the table entry times a DIFFERENCE of
                // nodal values: a constant field has exactly zero gradient on any mesh
                const float vb_ = fmaf(bx0, Bm.vc, bx1 * Bm.vn), vt_ = fmaf(bx0, Tp.vc, bx1 * Tp.vn);
                if constexpr (WNU) {
                    const float vx = dx1 * fmaf(by0, Bm.vn - Bm.vc, by1 * (Tp.vn - Tp.vc));
                    const float vy = dy1 * (vt_ - vb_);
                    float ux = vx, uy = vy;
                    if constexpr (HASV) {
                        ux = dx1 * fmaf(by0, Bm.un - Bm.uc, by1 * (Tp.un - Tp.uc));
                        uy = dy1 * (fmaf(bx0, Tp.uc, bx1 * Tp.un) - fmaf(bx0, Bm.uc, bx1 * Bm.un));
                    }
                    const float s = wq * fmaf(vx, ux, vy * uy);
                    const float t0 = by0 * s, t1 = by1 * s;
                    an[0] = fmaf(bx0, t0, an[0]);
                    an[1] = fmaf(bx1, t0, an[1]);
                    an[2] = fmaf(bx0, t1, an[2]);
                    an[3] = fmaf(bx1, t1, an[3]);
                }
                if constexpr (WF) {
                    const float s = wq * fmaf(by0, vb_, by1 * vt_);
                    const float t0 = by0 * s, t1 = by1 * s;
                    af[0] = fmaf(bx0, t0, af[0]);
                    af[1] = fmaf(bx1, t0, af[1]);
                    af[2] = fmaf(bx0, t1, af[2]);
                    af[3] = fmaf(bx1, t1, af[3]);
                }
            }
        }
        const bool ok = L.elem_x && e >= 0 && e < p.nely;
        // an output that is not wanted: zeros, so that the march carries a defined value
        bot[0] = bot[1] = top[0] = top[1] = 0.f;
        if constexpr (WNU) q1_owner_handover(ok, an, bot[0], top[0]);
        if constexpr (WF) q1_owner_handover(ok, af, bot[1], top[1]);
    };

    // node row e of the wanted outputs
    auto finish = [&](int e, const Row&, const float (&carry)[2], const float (&bot)[2]) {
        const unsigned rowoff = (unsigned)e * (unsigned)nx + L.qc;
        if constexpr (WNU) {
            if (L.owner) st_at<float>(onu, rowoff, snu * (carry[0] + bot[0]));
        }
        if constexpr (WF) {
            if (L.owner) st_at<float>(of, rowoff, sf * (carry[1] + bot[1]));
        }
    };

    const int j0 = strip * p.rows_per_strip, j1 = min(j0 + p.rows_per_strip, ny);
    constexpr int NF = 2;
#include "q1_owner_march.inl"
}

// ---- 3-D Q1, the plain form ------------------------------------------------------------------------------------------------------
template <int NGP, bool HASV, int MK, bool BCF>
__global__ void __launch_bounds__(256) coef_grad3d_kernel(const CoefGradParams p) {
    constexpr bool MASK = MK != CG_MK_NONE;
    using MT = typename CgMaskT<MK>::type;
    const int nx = p.nx, ny = p.ny, nz = p.nz;
    const int cx = (nx + 63) >> 6;                  // 64-node pieces of a node row
    const int i = ((int)blockIdx.x % cx) * 64 + (int)threadIdx.x;
    const int j = (int)blockIdx.x / cx, k = (int)blockIdx.y;
    const int b = blockIdx.z;
    const bool live = i < nx;
    const int64_t nps = (int64_t)nx * ny * nz;
    const float* ub = p.u + (int64_t)b * nps;
    const float* vb = HASV ? p.v + (int64_t)b * nps : ub;
    const MT* mp[2];
    const float* bcfb[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        mp[c] = MASK ? reinterpret_cast<const MT*>(p.mask[c]) + (p.mask_batched[c] ? (int64_t)b * nps : 0) : nullptr;
        bcfb[c] = BCF ? p.bcf[c] + (p.bcf_batched[c] ? (int64_t)b * nps : 0) : ub;
    }
    float sc = 1.f;
    if (p.in_scale) sc = p.in_scale[0];

    // the 27 substituted values around the node (indices clamped into the mesh: a clamped value only feeds an element that does not exist)
    float U[3][3][3], V[3][3][3];
#pragma unroll
    for (int dz_ = 0; dz_ < 3; ++dz_)
#pragma unroll
        for (int dy_ = 0; dy_ < 3; ++dy_)
#pragma unroll
            for (int dx_ = 0; dx_ < 3; ++dx_) {
                const unsigned off = ((unsigned)min(max(k + dz_ - 1, 0), nz - 1) * (unsigned)ny + (unsigned)min(max(j + dy_ - 1, 0), ny - 1)) * (unsigned)nx +
                                     (unsigned)min(max(i + dx_ - 1, 0), nx - 1);
                float uv = ld_at<float>(ub, off), vv = 0.f;
                if constexpr (HASV) vv = ld_at<float>(vb, off);
                if constexpr (MASK) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const bool fx = cg_set<MK>(ld_at<MT>(mp[c], off));
                        float bv = p.bcv[c];
                        if constexpr (BCF) {
                            const float bf = ld_at<float>(bcfb[c], off);
                            bv = p.bcf_set[c] ? bf : bv;
                        }
                        uv = fx ? bv : uv;
                        vv = fx ? 0.f : vv;
                    }
                }
                U[dz_][dy_][dx_] = uv;
                V[dz_][dy_][dx_] = HASV ? vv : uv;
            }

    // the 1-D tables in LDS: the Gauss-point loops below are rolled and index them at run time
    __shared__ float tb[3][4][2], td[3][4][2], tw[4];
    if (threadIdx.x < 8) {
        const int g = (int)threadIdx.x >> 1, l = (int)threadIdx.x & 1;
        tb[0][g][l] = p.tb.bx[g][l]; td[0][g][l] = p.tb.dx[g][l];
        tb[1][g][l] = p.tb.by[g][l]; td[1][g][l] = p.tb.dy[g][l];
        tb[2][g][l] = p.bz[g][l]; td[2][g][l] = p.dz[g][l];
        if (l == 0) tw[g] = p.w1[g];
    }
    __syncthreads();

    float gn = 0.f, gf = 0.f;
    // the node's <= 8 elements in the fixed order z, y, x; in element (k + ez - 1, j + ey - 1, i + ex - 1) the node is local node (1 - ez, 1 - ey, 1 - ex).
    // The element loops are unrolled (register indices of U, V are static), the Gauss-point loops are not.
#pragma unroll
    for (int ez = 0; ez < 2; ++ez)
#pragma unroll
        for (int ey = 0; ey < 2; ++ey)
#pragma unroll
            for (int ex = 0; ex < 2; ++ex) {
                const bool ok = (i + ex - 1) >= 0 && (i + ex - 1) < p.nelx && (j + ey - 1) >= 0 && (j + ey - 1) < p.nely && (k + ez - 1) >= 0 &&
                                (k + ez - 1) < p.nelz;
                float en = 0.f, ef = 0.f;
#pragma unroll 1
                for (int kg = 0; kg < NGP; ++kg) {
                    const float bz0 = tb[2][kg][0], bz1 = tb[2][kg][1], dz1 = td[2][kg][1];
#pragma unroll 1
                    for (int jg = 0; jg < NGP; ++jg) {
                        const float by0 = tb[1][jg][0], by1 = tb[1][jg][1], dy1 = td[1][jg][1];
                        const float wzy = tw[kg] * tw[jg];
                        const float nzy = (ez ? bz0 : bz1) * (ey ? by0 : by1);
#pragma unroll 1
                        for (int ig = 0; ig < NGP; ++ig) {
                            const float bx0 = tb[0][ig][0], bx1 = tb[0][ig][1], dx1 = td[0][ig][1];
                            // value and gradient of a field at the point from the element's eight nodes
                            auto eval = [&](const float (&F)[3][3][3], float& val, float& fx, float& fy, float& fz) {
                                float vx[2][2], gx[2][2];
#pragma unroll
                                for (int lz = 0; lz < 2; ++lz)
#pragma unroll
                                    for (int ly = 0; ly < 2; ++ly) {
                                        const float f0 = F[ez + lz][ey + ly][ex], f1 = F[ez + lz][ey + ly][ex + 1];
                                        vx[lz][ly] = fmaf(bx0, f0, bx1 * f1);
                                        gx[lz][ly] = dx1 * (f1 - f0);          // N0' = -N1': a constant field has exactly zero gradient
                                    }
                                const float v0 = fmaf(by0, vx[0][0], by1 * vx[0][1]), v1 = fmaf(by0, vx[1][0], by1 * vx[1][1]);
                                val = fmaf(bz0, v0, bz1 * v1);
                                fz = dz1 * (v1 - v0);
                                fx = fmaf(bz0, fmaf(by0, gx[0][0], by1 * gx[0][1]), bz1 * fmaf(by0, gx[1][0], by1 * gx[1][1]));
                                fy = dy1 * fmaf(bz0, vx[0][1] - vx[0][0], bz1 * (vx[1][1] - vx[1][0]));
                            };
                            float vg, vx_, vy_, vz_;
                            eval(V, vg, vx_, vy_, vz_);
                            float ux_ = vx_, uy_ = vy_, uz_ = vz_;
                            if constexpr (HASV) {
                                float ug;
                                eval(U, ug, ux_, uy_, uz_);
                            }
                            const float wn = wzy * tw[ig] * nzy * (ex ? bx0 : bx1);
                            en = fmaf(wn, fmaf(vx_, ux_, fmaf(vy_, uy_, vz_ * uz_)), en);
                            ef = fmaf(wn, vg, ef);
                        }
                    }
                }
                gn += ok ? en : 0.f;
                gf += ok ? ef : 0.f;
            }
    if (live) {
        const unsigned off = ((unsigned)k * (unsigned)ny + (unsigned)j) * (unsigned)nx + (unsigned)i;
        if (p.gnu) st_at<float>(p.gnu + (int64_t)b * nps, off, p.a_nu * sc * gn);
        if (p.gf) st_at<float>(p.gf + (int64_t)b * nps, off, p.a_f * sc * gf);
    }
}

#define CG2_LAUNCH(...) hipLaunchKernelGGL((coef_grad2d_kernel<__VA_ARGS__>), grid, block, 0, s, pp)
#define CG3_LAUNCH(...) hipLaunchKernelGGL((coef_grad3d_kernel<__VA_ARGS__>), grid, block, 0, s, pp)

// form: 0 no condition, 1 / 2 uint8 / fp32 images with constants, 3 / 4 the same with a value field
template <int NGP, bool HASV, int WANT>
static void cg2_launch_form(const CoefGradParams& pp, int form, dim3 grid, dim3 block, hipStream_t s) {
    constexpr bool NEEDU = (WANT & 1) || !HASV;
    if constexpr (NEEDU) {
        if (form == 3) { CG2_LAUNCH(NGP, HASV, WANT, CG_MK_U8, true); return; }
        if (form == 4) { CG2_LAUNCH(NGP, HASV, WANT, CG_MK_F32, true); return; }
    }
    if (form == 0) CG2_LAUNCH(NGP, HASV, WANT, CG_MK_NONE, false);
    else if (form == 1 || form == 3) CG2_LAUNCH(NGP, HASV, WANT, CG_MK_U8, false);
    else CG2_LAUNCH(NGP, HASV, WANT, CG_MK_F32, false);
}

template <int NGP>
static void cg2_launch_ngp(const CoefGradParams& pp, int form, int want, dim3 grid, dim3 block, hipStream_t s) {
    if (pp.v) {
        if (want == 1) cg2_launch_form<NGP, true, 1>(pp, form, grid, block, s);
        else if (want == 2) cg2_launch_form<NGP, true, 2>(pp, form, grid, block, s);
        else cg2_launch_form<NGP, true, 3>(pp, form, grid, block, s);
    } else {
        if (want == 1) cg2_launch_form<NGP, false, 1>(pp, form, grid, block, s);
        else if (want == 2) cg2_launch_form<NGP, false, 2>(pp, form, grid, block, s);
        else cg2_launch_form<NGP, false, 3>(pp, form, grid, block, s);
    }
}

template <int NGP, bool HASV>
static void cg3_launch_form(const CoefGradParams& pp, int form, dim3 grid, dim3 block, hipStream_t s) {
    switch (form) {
        case 0: CG3_LAUNCH(NGP, HASV, CG_MK_NONE, false); return;
        case 1: CG3_LAUNCH(NGP, HASV, CG_MK_U8, false); return;
        case 2: CG3_LAUNCH(NGP, HASV, CG_MK_F32, false); return;
        case 3: CG3_LAUNCH(NGP, HASV, CG_MK_U8, true); return;
        default: CG3_LAUNCH(NGP, HASV, CG_MK_F32, true); return;
    }
}

template <int NGP>
static void cg3_launch_ngp(const CoefGradParams& pp, int form, dim3 grid, dim3 block, hipStream_t s) {
    if (pp.v) cg3_launch_form<NGP, true>(pp, form, grid, block, s);
    else cg3_launch_form<NGP, false>(pp, form, grid, block, s);
}

constexpr int COEF_GRAD_MIN_ROWS = 8;          // shortest strip of the default plan: a strip recomputes one halo element row

// The plan of the flow operators; "PLAN2D" = "T,E,R[,W]" overrides the node rows per strip with its R (the other numbers belong to the
// Poisson kernels).  The results do not depend on it.
static Flow2dGeom coef_grad_plan(const dn_mesh* m) {
    Flow2dGeom g = flow2d_plan(m, COEF_GRAD_MIN_ROWS);
    if (const char* s = config(CFG_PLAN2D)) {
        int t = 0, e = 0, r = 0;
        if (std::sscanf(s, "%d,%d,%d", &t, &e, &r) == 3 && r >= 1) {
            g.R = std::min(r, (int)m->ny);
            g.strips = (m->ny + g.R - 1) / g.R;
            const int64_t waves = (int64_t)g.chunks * g.strips;
            g.wpb = (int)std::min<int64_t>(waves, 4);
            g.gx = (int)((waves + g.wpb - 1) / g.wpb);
        }
    }
    return g;
}

}  // namespace dn

using namespace dn;

extern "C" int dn_poisson_coef_grad(const dn_mesh* m, const dn_coef_grad_args* a, void* stream) {
    if (!m) return DN_E_BADARG;
    if (m->nsd != 2 && m->nsd != 3) return DN_E_UNSUPPORTED;
    if (m->degree != 1 || m->ngp < 2 || m->ngp > 4) return DN_E_UNSUPPORTED;
    if (m->nsd == 2) {
        const int rc = flow2d_validate(m);
        if (rc) return rc;
    } else {
        if (m->batch < 1 || m->batch > 65535 || m->nx < 2 || m->ny < 2 || m->nz < 2) return DN_E_BADARG;
        if ((int64_t)m->nx * m->ny * m->nz >= (1ll << 30) || m->nz > 65535) return DN_E_UNSUPPORTED;
    }
    if (!a || !a->u) return DN_E_BADARG;
    if (!a->g_nu && !a->g_f) return DN_E_BADARG;

    CoefGradParams pp = {};
    int kind = -1, nbc = 0;
    bool bcf = false;
    for (int k = 0; k < 2; ++k) {
        const dn_dirichlet& d = a->bc[k];
        if (d.mask_kind == DN_MASK_BITS || d.mask_kind == DN_MASK_BOX) return DN_E_UNSUPPORTED;
        if (d.mask_kind != DN_MASK_F32 && d.mask_kind != DN_MASK_U8) return DN_E_BADARG;
        if ((d.mask_batched | d.field_batched) & ~1) return DN_E_BADARG;
        if (!d.mask) {
            if (d.field) return DN_E_BADARG;                                   // a value field without a condition
            continue;
        }
        if (kind >= 0 && kind != d.mask_kind) return DN_E_UNSUPPORTED;         // two images of different formats: convert one
        kind = d.mask_kind;
        pp.mask[nbc] = d.mask;
        pp.mask_batched[nbc] = d.mask_batched;
        pp.bcf[nbc] = d.field ? d.field : a->u;
        pp.bcf_batched[nbc] = d.field ? d.field_batched : 1;
        pp.bcf_set[nbc] = d.field ? 1 : 0;
        pp.bcv[nbc] = d.value;
        bcf = bcf || d.field;
        ++nbc;
    }
    if (nbc == 0) {
        pp.bcf[0] = pp.bcf[1] = a->u;
        pp.bcf_batched[0] = pp.bcf_batched[1] = 1;
    } else if (nbc == 1) {                                                     // the condition twice: a substitution is idempotent
        pp.mask[1] = pp.mask[0];
        pp.mask_batched[1] = pp.mask_batched[0];
        pp.bcf[1] = pp.bcf[0];
        pp.bcf_batched[1] = pp.bcf_batched[0];
        pp.bcf_set[1] = pp.bcf_set[0];
        pp.bcv[1] = pp.bcv[0];
    }
    const int want = (a->g_nu ? 1 : 0) | (a->g_f ? 2 : 0);
    const bool needu = (want & 1) || !a->v;
    int form = nbc == 0 ? 0 : (kind == DN_MASK_U8 ? 1 : 2);
    if (form && bcf && (needu || m->nsd == 3)) form += 2;

    pp.u = a->u;
    pp.v = a->v;
    pp.in_scale = a->in_scale;
    pp.gnu = a->g_nu;
    pp.gf = a->g_f;
    const int ngp = m->ngp;
    q1_tables_fill(pp.tb, m, a->wscale);       // 3-D too: its kernel reads bx .. dy of it and never wg
    for (int ig = 0; ig < 4; ++ig)
        for (int i = 0; i < 2; ++i) {
            pp.bz[ig][i] = pp.tb.bx[ig][i];
            pp.dz[ig][i] = ig < ngp ? (float)(m->dbasis[ig][i] * (double)m->scale[2]) : 0.f;
        }
    for (int ig = 0; ig < 4; ++ig) pp.w1[ig] = ig < ngp ? m->gpw[ig] : 0.f;
    pp.nx = m->nx; pp.ny = m->ny; pp.nz = m->nsd == 3 ? m->nz : 1;
    pp.nelx = m->nx - 1; pp.nely = m->ny - 1; pp.nelz = pp.nz - 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);

    if (m->nsd == 2) {
        pp.a_nu = a->a_nu;
        pp.a_f = a->a_f;
        const Flow2dGeom g = coef_grad_plan(m);
        pp.chunks = g.chunks; pp.rows_per_strip = g.R; pp.strips = g.strips;
        const dim3 grid(g.gx, m->batch), block(64 * g.wpb);
        switch (ngp) {
            case 2: cg2_launch_ngp<2>(pp, form, want, grid, block, s); break;
            case 3: cg2_launch_ngp<3>(pp, form, want, grid, block, s); break;
            default: cg2_launch_ngp<4>(pp, form, want, grid, block, s); break;
        }
    } else {
        pp.a_nu = a->a_nu * a->wscale;
        pp.a_f = a->a_f * a->wscale;
        const dim3 block(64), grid(((m->nx + 63) / 64) * m->ny, m->nz, m->batch);
        switch (ngp) {
            case 2: cg3_launch_ngp<2>(pp, form, grid, block, s); break;
            case 3: cg3_launch_ngp<3>(pp, form, grid, block, s); break;
            default: cg3_launch_ngp<4>(pp, form, grid, block, s); break;
        }
    }
    DN_LAUNCH_CHECK();
    return 0;
}
