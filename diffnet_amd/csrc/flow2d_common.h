// Shared by the two three-field 2-D flow operators (stokes.hip, navier_stokes.hip): everything that is not their mathematics.  The
// kernel parameters both use, the per-sample base pointers, the row loader, the Dirichlet test, the in_num / in_den scale (the wave's
// place in the launch, the lane's column and the hand-over between lanes: q1_owner_march.h, which transport.hip and
// poisson_coef_grad.hip share too); on the host the mesh check, the launch plan, the reduction workspace, the argument checks common to
// dn_stokes_args and dn_ns_args (same member names), their copy into the parameters and the (MASK, BCF, FGP) launch switch.
// Nothing here asks which operator it serves: what differs stays in the operator's own file, after or around these calls.
#pragma once
#include <algorithm>

#include "q1_owner_march.h"

namespace dn {

// StokesParams and NsParams derive from this
struct Flow2dParams {
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
    const float* in_num;                   // optional 3 + 3 device floats: the scale in_num[k] / in_den[k] (flow2d_in_scale)
    const float* in_den;
    float* out[3];
    double* part;                          // [3][nblocks] partial sums of squares (finish_sums3 in dn_reduce.h)
    unsigned* counter;
    double* sumsq;
    float* norms;
    int nx, ny, nelx, nely, chunks, rows_per_strip, strips, want_sums;
};

// A lane's column (Q1Lane, q1_owner_march.h) and the base pointers of its sample.  NX: extra node arrays a row carries (the caller sets xb)
template <int NX>
struct Flow2dLane : Q1Lane {
    const float* fb[3];
    const float* xb[NX ? NX : 1];
    const float* bcf[3];
    const float* mfp[3];
    const uint8_t* mbp[3];
    float* ob[3];
    const float* fg[2];
};

template <int NX>
__device__ __forceinline__ void flow2d_lane(const Flow2dParams& p, int chunk, int lane, Flow2dLane<NX>& L) {
    q1_lane(chunk, lane, p.nx, p.nelx, p.nely, L);
}

// Base pointers of field k (k < 3) in sample b.  The kernels call it in a loop over k of their own: until that loop is unrolled the
// parameters are indexed at run time in the kernel, which keeps the compiler from splitting its copy of them into registers at entry
// (it then reads each member from the kernel-argument segment where it is used; loading all of them up front costs SGPRs, spilled
// into VGPRs in the larger kernels)
template <int G, int NX>
__device__ __forceinline__ void flow2d_field_base(const Flow2dParams& p, int b, int k, Flow2dLane<NX>& L) {
    const int64_t nps = (int64_t)p.nx * p.ny;
    L.fb[k] = p.fld[k] + (int64_t)b * nps;
    L.bcf[k] = p.bcf[k] ? p.bcf[k] + (p.bcf_batched[k] ? (int64_t)b * nps : 0) : L.fb[k];
    const int64_t mo = p.mask_batched[k] ? (int64_t)b * nps : 0;
    L.mfp[k] = reinterpret_cast<const float*>(p.mask[k]) + (p.mask_kind[k] == 2 ? mo : 0);
    L.mbp[k] = reinterpret_cast<const uint8_t*>(p.mask[k]) + (p.mask_kind[k] == 1 ? mo : 0);
    L.ob[k] = p.out[k] ? p.out[k] + (int64_t)b * nps : nullptr;
    if (k < 2) L.fg[k] = p.fgp[k] ? p.fgp[k] + (p.fgp_batched[k] ? (int64_t)b * G * L.nel : 0) : nullptr;
}

// in_num[k] / in_den[k]: the cotangent of the norms over the norms (the VJP of ||R_k||), torch's convention at ||R_k|| == 0: zero
__device__ __forceinline__ void flow2d_in_scale(const Flow2dParams& p, float (&s)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = 1.f;
    if (p.in_num) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float den = p.in_den[k];
            s[k] = den > 0.f ? p.in_num[k] / den : (den == den ? 0.f : den);
        }
    }
}

// Raw loads of one node row r (clamped into the mesh) and, with the Gauss-point forcing, of the element layer r - 1 under it
template <int G, bool MASK, bool BCF, bool FGP, int NX>
struct Flow2dRaw {
    float v[3];
    float x[NX ? NX : 1];
    float mf[MASK ? 3 : 1];
    uint8_t mb[MASK ? 3 : 1];
    float bf[BCF ? 3 : 1];
    float f[FGP ? 2 : 1][FGP ? G : 1];
};

template <int G, bool MASK, bool BCF, bool FGP, int NX>
__device__ __forceinline__ void flow2d_issue(const Flow2dParams& p, const Flow2dLane<NX>& L, int r, Flow2dRaw<G, MASK, BCF, FGP, NX>& w) {
    const unsigned rowoff = (unsigned)min(max(r, 0), p.ny - 1) * (unsigned)p.nx + L.qc;
#pragma unroll
    for (int k = 0; k < 3; ++k) w.v[k] = ld_at<float>(L.fb[k], rowoff);
#pragma unroll
    for (int k = 0; k < NX; ++k) w.x[k] = ld_at<float>(L.xb[k], rowoff);
    if constexpr (MASK) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            w.mf[k] = 0.f;
            w.mb[k] = 0;
            if (p.mask_kind[k] == 2) w.mf[k] = ld_at<float>(L.mfp[k], rowoff);
            else if (p.mask_kind[k] == 1) w.mb[k] = ld_at<uint8_t>(L.mbp[k], rowoff);
        }
    }
    if constexpr (BCF) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            w.bf[k] = 0.f;
            if (p.bcf[k]) w.bf[k] = ld_at<float>(L.bcf[k], rowoff);
        }
    }
    if constexpr (FGP) {
        const unsigned eoff = (unsigned)min(max(r - 1, 0), p.nely - 1) * (unsigned)p.nelx + L.qe;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int g = 0; g < G; ++g) w.f[k][g] = L.fg[k] ? ld_at<float>(L.fg[k], eoff + (unsigned)(g * L.nel)) : 0.f;
    }
}

// is field k of a landed row a Dirichlet node?  (MASK kernels only)
template <class Raw>
__device__ __forceinline__ bool flow2d_fixed(const Flow2dParams& p, const Raw& w, int k) {
    return p.mask_kind[k] == 2 ? (w.mf[k] >= 0.5f) : (p.mask_kind[k] == 1 ? (w.mb[k] != 0) : false);
}

// ---- host ----

struct Flow2dGeom { int chunks, strips, R, wpb, gx; };

static inline int flow2d_validate(const dn_mesh* m) {
    if (!m) return DN_E_BADARG;
    if (m->nsd != 2 || m->degree != 1 || m->ngp < 2 || m->ngp > 4) return DN_E_UNSUPPORTED;
    if (m->batch < 1 || m->batch > 65535 || m->nx < 2 || m->ny < 2) return DN_E_BADARG;
    const int64_t nps = (int64_t)m->nx * m->ny, nel = (int64_t)(m->nx - 1) * (m->ny - 1);
    if (nps >= (1ll << 30) || nel * m->ngp * m->ngp >= (1ll << 30)) return DN_E_UNSUPPORTED;     // 32-bit byte offsets within a sample
    return 0;
}

// One wave per (62-column chunk, strip of R node rows, sample); strips as short as min_rows until the launch has ~4096 waves (16 per CU:
// the kernels stream their rows from HBM, and the latency of a row's loads is hidden by the other waves of the SIMD and the prefetch).
static inline Flow2dGeom flow2d_plan(const dn_mesh* m, int min_rows) {
    Flow2dGeom g;
    g.chunks = (m->nx + FLOW2D_OWNERS - 1) / FLOW2D_OWNERS;
    const int64_t per_row = (int64_t)g.chunks * m->batch;
    int strips = (int)std::min<int64_t>((4096 + per_row - 1) / per_row, (m->ny + min_rows - 1) / min_rows);
    strips = std::max(strips, 1);
    g.R = (m->ny + strips - 1) / strips;
    g.strips = (m->ny + g.R - 1) / g.R;
    const int waves = g.chunks * g.strips;
    g.wpb = std::min(waves, 4);
    g.gx = (waves + g.wpb - 1) / g.wpb;
    return g;
}

static inline int64_t flow2d_workspace_bytes(const Flow2dGeom& g, int batch) {
    return DN_WS_HEADER + (int64_t)(3 * sizeof(double)) * g.gx * batch;
}

// the DN_E_BADARG checks common to dn_stokes_args and dn_ns_args
template <class Args>
static int flow2d_check_args(const Args* a) {
    if (!a || !a->u || !a->v || !a->p) return DN_E_BADARG;
    if (!a->out[0] && !a->out[1] && !a->out[2] && !a->sumsq && !a->norms) return DN_E_BADARG;
    if ((a->in_num != nullptr) != (a->in_den != nullptr)) return DN_E_BADARG;
    for (int k = 0; k < 3; ++k) {
        if ((a->mask_is_u8[k] | a->mask_batched[k] | a->bc_field_batched[k]) & ~1) return DN_E_BADARG;
        if (a->bc_field[k] && !a->bc_mask[k]) return DN_E_BADARG;           // a value field without a condition
    }
    for (int k = 0; k < 2; ++k)
        if (a->f_batched[k] & ~1) return DN_E_BADARG;
    return 0;
}

// ... and, after the operator's own DN_E_BADARG checks, the workspace of a reducing call
template <class Args>
static int flow2d_check_workspace(const Args* a, const Flow2dGeom& g, int batch) {
    const bool want_red = a->sumsq || a->norms;
    if (want_red && (!a->workspace || a->workspace_bytes < flow2d_workspace_bytes(g, batch))) return DN_E_WORKSPACE;
    return 0;
}

template <class Args>
static void flow2d_fill(Flow2dParams& pp, const dn_mesh* m, const Args* a, const Flow2dGeom& g) {
    pp.fld[0] = a->u; pp.fld[1] = a->v; pp.fld[2] = a->p;
    for (int k = 0; k < 3; ++k) {
        pp.mask[k] = a->bc_mask[k];
        pp.mask_kind[k] = !a->bc_mask[k] ? 0 : (a->mask_is_u8[k] ? 1 : 2);
        pp.mask_batched[k] = a->mask_batched[k];
        pp.bcf[k] = a->bc_field[k];
        pp.bcf_batched[k] = a->bc_field_batched[k];
        pp.bcv[k] = a->bc_value[k];
        pp.out[k] = a->out[k];
    }
    for (int k = 0; k < 2; ++k) {
        pp.fgp[k] = a->f_gp[k];
        pp.fgp_batched[k] = a->f_batched[k];
        pp.fconst[k] = a->f_gp[k] ? 0.f : a->f_value[k];
    }
    pp.in_num = a->in_num;
    pp.in_den = a->in_den;
    pp.counter = reinterpret_cast<unsigned*>(a->workspace);
    pp.part = a->workspace ? reinterpret_cast<double*>(reinterpret_cast<char*>(a->workspace) + DN_WS_HEADER) : nullptr;
    pp.sumsq = a->sumsq;
    pp.norms = a->norms;
    pp.nx = m->nx; pp.ny = m->ny;
    pp.nelx = m->nx - 1; pp.nely = m->ny - 1;
    pp.chunks = g.chunks; pp.rows_per_strip = g.R; pp.strips = g.strips;
    pp.want_sums = (a->sumsq || a->norms) ? 1 : 0;
}

// Launch of one kernel family: Family::launch<MASK, BCF, FGP>(grid, block, stream, pp) picks its instantiation.  MASK: any condition,
// BCF: any value field, FGP: any Gauss-point forcing -- read from the filled parameters
template <class Family, class Params>
static void flow2d_launch(const Params& pp, const Flow2dGeom& g, int batch, hipStream_t s) {
    const dim3 grid(g.gx, batch), block(64 * g.wpb);
    const bool mask = pp.mask[0] || pp.mask[1] || pp.mask[2], bcf = pp.bcf[0] || pp.bcf[1] || pp.bcf[2];
    const int sel = (mask ? (bcf ? 2 : 1) : 0);
    if (pp.fgp[0] || pp.fgp[1]) {
        switch (sel) {
            case 0: Family::template launch<false, false, true>(grid, block, s, pp); return;
            case 1: Family::template launch<true, false, true>(grid, block, s, pp); return;
            default: Family::template launch<true, true, true>(grid, block, s, pp); return;
        }
    }
    switch (sel) {
        case 0: Family::template launch<false, false, false>(grid, block, s, pp); return;
        case 1: Family::template launch<true, false, false>(grid, block, s, pp); return;
        default: Family::template launch<true, true, false>(grid, block, s, pp); return;
    }
}

}  // namespace dn
