// Element-owner march of the 2-D Q1 residual kernels (navier_stokes.hip, transport.hip, the 2-D half of poisson_coef_grad.hip) and what
// surrounds it that is not an operator's mathematics: the wave's place in the launch, the lane's place in the mesh, the Gauss-point
// evaluation of a nodal field, the flux-form scatter, the hand-over to the neighbour lane and the basis tables.  The march itself is the
// text of q1_owner_march.inl, which the three kernels include in their bodies.
//
// One wave = 62 owner columns + two ghost lanes; lane q owns node column q and the element to its right.  A lane marches the node rows of
// a strip, loads every node row once (the x neighbour comes over ds_bpermute), computes its element's four local contributions per output,
// hands the two right-hand ones to its neighbour lane (q1_owner_handover) and carries the top pair in registers into the next element row.
// A strip recomputes one halo element row under it, so every output node is written once, by its owner lane, with the same additions in
// any launch plan: no atomics on the data path, results bitwise independent of the plan and of the other samples of the batch.
//
// Nothing here receives a kernel's parameter struct: the march calls the kernel's closures, the helpers see floats and ints (a helper that
// reads the parameters makes the compiler split its copy of them into SGPRs at kernel entry: profiles/flow2d_refactor.txt).
#pragma once
#include "dn_reduce.h"

namespace dn {

constexpr int FLOW2D_OWNERS = 62;          // owner lanes per wave (lanes 1 .. 62); lanes 0 and 63 are ghosts that only supply the x halo

// One wave per (62-column chunk, strip of node rows, sample): the wave's chunk and strip (strip >= p.strips: a wave of the last
// workgroup with nothing to do) and the lane.  Params: anything with `chunks`
template <class Params>
__device__ __forceinline__ void flow2d_wave(const Params& p, int& lane, int& chunk, int& strip) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    lane = (int)threadIdx.x & 63;
    const int wid = (int)blockIdx.x * ((int)blockDim.x >> 6) + wave;
    chunk = wid % p.chunks;
    strip = wid / p.chunks;
}

// A lane's place in the mesh
struct Q1Lane {
    int q;                                 // node column of the lane
    bool owner;
    unsigned qc;                           // q clamped into the mesh
    bool elem_x;                           // the element to the right of the lane's column exists
    unsigned qe;                           // its column, clamped
    int nel;
};

__device__ __forceinline__ void q1_lane(int chunk, int lane, int nx, int nelx, int nely, Q1Lane& L) {
    L.q = chunk * FLOW2D_OWNERS + lane - 1;
    L.owner = lane >= 1 && lane <= FLOW2D_OWNERS && L.q < nx;
    L.qc = (unsigned)min(max(L.q, 0), nx - 1);
    L.elem_x = L.q >= 0 && L.q < nelx;
    L.qe = (unsigned)min(max(L.q, 0), nelx - 1);
    L.nel = nelx * nely;
}

// value and derivatives at one point from the element's four nodal values (local node ly * 2 + lx)
__device__ __forceinline__ void q1_eval(float bx0, float bx1, float dx0, float dx1, float by0, float by1, float dy0, float dy1,
                                        float f0, float f1, float f2, float f3, float& val, float& fx, float& fy) {
    const float vb = fmaf(bx0, f0, bx1 * f1), vt = fmaf(bx0, f2, bx1 * f3);
    const float db = fmaf(dx0, f0, dx1 * f1), dt = fmaf(dx0, f2, dx1 * f3);
    val = fmaf(by0, vb, by1 * vt);
    fx = fmaf(by0, db, by1 * dt);
    fy = fmaf(dy0, vb, dy1 * vt);
}

// flux form at one point: adds w (N_a A + Nx_a B + Ny_a C) into the element's four local nodes
__device__ __forceinline__ void q1_flux_scatter(float bx0, float bx1, float dx0, float dx1, float by0, float by1, float dy0, float dy1,
                                                float wq, float A, float B, float C, float (&acc)[4]) {
    const float Aw = wq * A, Bw = wq * B, Cw = wq * C;
    const float s0 = fmaf(by0, Aw, dy0 * Cw), s1 = fmaf(by1, Aw, dy1 * Cw);     // per ly: N_ly A + N'_ly C
    const float t0 = by0 * Bw, t1 = by1 * Bw;
    acc[0] = fmaf(bx0, s0, fmaf(dx0, t0, acc[0]));
    acc[1] = fmaf(bx1, s0, fmaf(dx1, t0, acc[1]));
    acc[2] = fmaf(bx0, s1, fmaf(dx0, t1, acc[2]));
    acc[3] = fmaf(bx1, s1, fmaf(dx1, t1, acc[3]));
}

// The hand-over of an element's four local contributions c (already zero where the element does not exist): the node's own element
// (right) as local node lx = 0, the left neighbour's element as lx = 1
__device__ __forceinline__ void q1_owner_handover(const float (&c)[4], float& bot, float& top) {
    bot = c[0] + __shfl_up(c[1], 1, 64);
    top = c[2] + __shfl_up(c[3], 1, 64);
}

// ... of acc where the element exists (ok), of zeros where it does not
__device__ __forceinline__ void q1_owner_handover(bool ok, const float (&acc)[4], float& bot, float& top) {
    float c[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) c[a] = ok ? acc[a] : 0.f;
    q1_owner_handover(c, bot, top);
}

// The 1-D Q1 tables at the Gauss points: a member (tb) of the kernels' parameter structs
struct Q1Tables {
    float bx[4][2], dx[4][2];              // 1-D Q1 basis / derivative (times 2 / hx) at the Gauss points along x
    float by[4][2], dy[4][2];              // along y
    float wg[16];                          // wscale w_ig w_jg, point jg * ngp + ig
};

// ---- host ----

static inline void q1_tables_fill(Q1Tables& t, const dn_mesh* m, double wscale) {
    const int ngp = m->ngp;
    const double sx = m->scale[0], sy = m->scale[1];
    for (int ig = 0; ig < 4; ++ig)
        for (int i = 0; i < 2; ++i) {
            const bool in = ig < ngp;
            t.bx[ig][i] = in ? m->basis[ig][i] : 0.f;
            t.by[ig][i] = in ? m->basis[ig][i] : 0.f;
            t.dx[ig][i] = in ? (float)(m->dbasis[ig][i] * sx) : 0.f;
            t.dy[ig][i] = in ? (float)(m->dbasis[ig][i] * sy) : 0.f;
        }
    for (int gq = 0; gq < 16; ++gq) {
        const int ig = gq % ngp, jg = gq / ngp;
        t.wg[gq] = gq < ngp * ngp ? (float)(wscale * m->gpw[ig] * m->gpw[jg]) : 0.f;
    }
}

}  // namespace dn
