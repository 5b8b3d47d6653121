// Shared by the element-march operators on structured 2-D Q_P meshes (strongform.hip, fosls.hip, helmholtz.hip, eikonal.hip): everything
// that is not their mathematics.  The kernel parameters they all use and the block sums of the reduction tail (the march itself is the
// kernel body of elem2d_march.inl); on the host the mesh check, the launch plan, the reduction workspace, the argument checks their
// argument structs have in common (same member names), the fill of the shared parameters and the (degree, rule) x FK x (MASK, BCF)
// launch switch.  Nothing here asks which operator it serves: what differs comes in through the operator's `Op` (device) and `Family`
// (host) types.
//
// The mapping is the element form of the FSDT kernel (fsdt.hip has the reasons): a thread owns one element column of a strip and marches
// over element rows; the contribution to the node column shared with the right neighbour goes through a double-buffered LDS slot;
// strip and chunk seams are closed by recomputing one layer / one column.  No atomics on the data path: every node is written once, by
// its owner, with the same additions in the same order under any launch plan and batch size.
#pragma once
#include <algorithm>
#include <cstdio>
#include <type_traits>

#include "dn_reduce.h"
#include "elem_args.h"

namespace dn {

// SfParams, FoParams, HhParams and EkParams derive from this
struct Elem2dParams {
    float b[4][4], dx[4][4], dy[4][4];     // 1-D tables at the Gauss points (derivatives scaled by 2/h)
    float w2[4][4];                        // w[jg] * w[ig] * wscale
    const float* f;                        // FK == 1: nodal forcing
    const float* fgp;                      // FK == 2: (B | 1, G, nely, nelx)
    int f_batched;
    const void* mask[2];
    int mask_kind[2];                      // 0: none, 1: uint8 (!= 0), 2: fp32 (> 0.5)
    int mask_batched[2];
    const float* bcf[2];
    int bcf_batched[2];
    float bcv[2];
    double* part;                          // [NS][nblocks] partial sums
    unsigned* counter;
    int nx, ny, nelx, nely, rows_per_strip, want_sums;
};

// An operator that wants the Dirichlet nodes of a landed row (eikonal.hip: the cotangent is zero there) has fixed_row(r, bits); for the
// others the march's call compiles to nothing
template <class Op, class = void>
struct elem2d_has_fixed_row : std::false_type {};
template <class Op>
struct elem2d_has_fixed_row<Op, std::void_t<decltype(&Op::fixed_row)>> : std::true_type {};

// block_sum of one value, block_sum2 of two (the same additions in the same order as before the kernels shared their tail); results in thread 0
__device__ __forceinline__ void elem2d_block_sums(double (&v)[1], double* scratch, int tid, int nthreads) { v[0] = block_sum(v[0], scratch, tid, nthreads); }
__device__ __forceinline__ void elem2d_block_sums(double (&v)[2], double* scratch, int tid, int nthreads) { block_sum2(v[0], v[1], scratch, tid, nthreads); }

// ---- host ----

static inline int elem2d_ceil_div(int a, int b) { return (a + b - 1) / b; }

struct Elem2dGeom { int T, chunks, R, strips; };

constexpr int ELEM2D_MIN_ROWS = 4;         // shortest strip the library chooses (element rows): a strip recomputes one layer

// Threads per workgroup by utilisation of the last chunk (wider wins at equal utilisation), then the strip height: enough waves for ~4
// per SIMD at the price of one recomputed layer per strip -- the rule of the FSDT element form, whose element these resemble.
// "PLAN_FSDT" ("T,R") overrides both, as it does there; the results do not depend on the plan.
static inline Elem2dGeom elem2d_plan(const dn_mesh* m) {
    Elem2dGeom g;
    const int P = m->degree;
    const int Q = (m->nx - 1) / P + 1;          // logical thread columns (one per element + the closing column)
    const int nely = (m->ny - 1) / P;
    double best = -1.0;
    g.T = 64; g.chunks = 1;
    for (int T = 64; T <= 256; T += 64) {
        const int chunks = Q <= T ? 1 : elem2d_ceil_div(Q - 1, T - 1);
        const double score = (double)Q / ((double)chunks * T) + 0.0003 * T;
        if (score > best) { best = score; g.T = T; g.chunks = chunks; }
    }
    const long long per_strip = (long long)g.chunks * m->batch * (g.T / 64);
    int R = 32;
    while (R > ELEM2D_MIN_ROWS && per_strip * elem2d_ceil_div(nely, R) < 4096) R /= 2;
    const char* e = config(CFG_PLAN_FSDT);
    int T, RR;
    if (e && sscanf(e, "%d,%d", &T, &RR) == 2 && T >= 64 && T <= 256 && T % 64 == 0 && RR >= 1) {
        g.T = T; R = RR;
        g.chunks = Q <= T ? 1 : elem2d_ceil_div(Q - 1, T - 1);
    }
    g.R = std::max(1, std::min(R, nely));
    g.strips = elem2d_ceil_div(nely, g.R);
    return g;
}

static inline int elem2d_validate(const dn_mesh* m) {
    if (!m || m->nsd != 2) return DN_E_BADARG;
    if (m->degree < 1 || m->degree > 3 || m->ngp < 2 || m->ngp > 4 || (m->degree > 1 && m->ngp < 3)) return DN_E_UNSUPPORTED;
    if (m->batch < 1 || m->batch > 65535 || m->nx < 2 || m->ny < 2) return DN_E_BADARG;
    if ((m->nx - 1) % m->degree || (m->ny - 1) % m->degree) return DN_E_BADARG;
    if ((int64_t)m->nx * m->ny >= (1ll << 30)) return DN_E_UNSUPPORTED;
    const int64_t nel = (int64_t)((m->nx - 1) / m->degree) * ((m->ny - 1) / m->degree);
    if (nel * m->ngp * m->ngp >= (1ll << 30) || (m->ny - 1) / m->degree > 65535) return DN_E_UNSUPPORTED;     // 32-bit offsets; grid.y
    return 0;
}

// nsums partial sums per workgroup, for an upper bound of the workgroups over every launch plan (one-wave chunks, one-row strips): the
// size does not change with "PLAN_FSDT"
static inline int64_t elem2d_workspace_bytes(const dn_mesh* m, int nsums) {
    const int P = m->degree;
    const int Q = (m->nx - 1) / P + 1, nely = (m->ny - 1) / P;
    const int64_t chunks = Q <= 64 ? 1 : elem2d_ceil_div(Q - 1, 63);
    return DN_WS_HEADER + nsums * (int64_t)sizeof(double) * chunks * nely * m->batch;
}

// The checks dn_strongform_args, dn_fosls_args, dn_helmholtz_args and dn_eikonal_args have in common, after the operator's own DN_E_BADARG checks: the
// forcing and the two conditions (elem_args.h), and the workspace of a call that reduces nsums sums (0: none)
template <class Args>
static int elem2d_check_args(const dn_mesh* m, const Args* a, int nsums) {
    if (const int rc = elem_check_conditions(a)) return rc;
    if (nsums && (!a->workspace || a->workspace_bytes < elem2d_workspace_bytes(m, nsums))) return DN_E_WORKSPACE;
    return 0;
}

template <class Args>
static void elem2d_fill(Elem2dParams& pp, const dn_mesh* m, const Args* a, const Elem2dGeom& g, bool want_sums) {
    const double sx = m->scale[0], sy = m->scale[1];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const bool in = i < m->ngp && j <= m->degree;
            pp.b[i][j] = in ? m->basis[i][j] : 0.f;
            pp.dx[i][j] = in ? (float)(m->dbasis[i][j] * sx) : 0.f;
            pp.dy[i][j] = in ? (float)(m->dbasis[i][j] * sy) : 0.f;
            pp.w2[i][j] = (i < m->ngp && j < m->ngp) ? m->gpw[i] * (m->gpw[j] * a->wscale) : 0.f;
        }
    elem_fill_conditions(pp, a);
    pp.nx = m->nx; pp.ny = m->ny;
    pp.nelx = (m->nx - 1) / m->degree; pp.nely = (m->ny - 1) / m->degree;
    pp.rows_per_strip = g.R;
    pp.want_sums = want_sums ? 1 : 0;
}

// Launch of one kernel family: Family::launch<P, NGP, MASK, BCF, FK>(grid, block, stream, pp) picks its instantiation (by the
// operator's own compile-time forms).  MASK: any condition, BCF: any value field, FK: the forcing -- read from the filled parameters
template <class Family, int P, int NGP, int FK>
static void elem2d_launch_mask(const typename Family::Params& pp, dim3 grid, dim3 block, hipStream_t s) {
    const bool mask = pp.mask[0] || pp.mask[1], bcf = pp.bcf[0] || pp.bcf[1];
    if (mask && bcf) Family::template launch<P, NGP, true, true, FK>(grid, block, s, pp);
    else if (mask) Family::template launch<P, NGP, true, false, FK>(grid, block, s, pp);
    else Family::template launch<P, NGP, false, false, FK>(grid, block, s, pp);
}

template <class Family, int P, int NGP>
void elem2d_launch_forms(const typename Family::Params& pp, dim3 grid, dim3 block, hipStream_t s) {
    if (pp.fgp) elem2d_launch_mask<Family, P, NGP, 2>(pp, grid, block, s);
    else if (pp.f) elem2d_launch_mask<Family, P, NGP, 1>(pp, grid, block, s);
    else elem2d_launch_mask<Family, P, NGP, 0>(pp, grid, block, s);
}

// The Q2 and Q3 instantiations of a family compile in translation units of their own (<operator>_q2.hip, <operator>_q3.hip):
// ELEM2D_DEGREE(extern, Family, 2) declares them where they are called, ELEM2D_DEGREE(, Family, 2) compiles them
#define ELEM2D_DEGREE(EXT, Family, P)                                                                             \
    EXT template void elem2d_launch_forms<Family, P, 3>(const Family::Params&, dim3, dim3, hipStream_t); \
    EXT template void elem2d_launch_forms<Family, P, 4>(const Family::Params&, dim3, dim3, hipStream_t)

template <class Family>
static void elem2d_launch(const dn_mesh* m, const typename Family::Params& pp, const Elem2dGeom& g, hipStream_t s) {
    const dim3 grid(g.chunks, g.strips, m->batch), block(g.T);
    switch (m->degree * 10 + m->ngp) {
        case 12: elem2d_launch_forms<Family, 1, 2>(pp, grid, block, s); break;
        case 13: elem2d_launch_forms<Family, 1, 3>(pp, grid, block, s); break;
        case 14: elem2d_launch_forms<Family, 1, 4>(pp, grid, block, s); break;
        case 23: elem2d_launch_forms<Family, 2, 3>(pp, grid, block, s); break;
        case 24: elem2d_launch_forms<Family, 2, 4>(pp, grid, block, s); break;
        case 33: elem2d_launch_forms<Family, 3, 3>(pp, grid, block, s); break;
        default: elem2d_launch_forms<Family, 3, 4>(pp, grid, block, s); break;
    }
}

}  // namespace dn
