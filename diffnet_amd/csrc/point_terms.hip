// Point-cloud terms on a Q1 mesh, 2-D or 3-D: evaluate u and its gradient at points, the scripts' penalty loss and its gradient.
//   u_p = sum_a N_a(xi_p) u_a        g_d = s_d sum_a d_d N_a(xi_p) u_a        over the 2^nsd nodes a of the point's element
//   value term    w_val sum_p (u_p - t_p)^2
//   normals term  w_nrm sum_p (g . n - 1)^2  ("dot")   or   w_nrm sum_p sum_d (g_d - n_d)^2  ("match")
// Reference forms (examples/): the four "+1" neighbour gathers and bf_1d_th / bf_1d_der_th products of
// poisson/single_instance/pc_poisson_disk.py (loss: sum (u_p - 1)^2), eiqonal/parametric/10_fixed_bc.py:186-208 and
// eiqonal/single_instance/05_3d_sphere_loss4.py:345-389 (value and "dot" terms), e01_curve_reconstruction.py:270 ("match").
//
// No data-dependent addressing is decided here: the Python plan (diffnet_amd/points.py) has classified every point into an element,
// clamped it and sorted the points by (sample, element); the kernels take the element ids, the local coordinates xi in [-1, 1]
// (structure of arrays, one array per axis) and, for the adjoint, the CSR offsets of the sorted list.  Element ids and offsets are
// still clamped into their ranges before they address anything.
//
// Forward: one thread per sorted point (grid-stride over at most PT_MAX_BLOCKS workgroups, so the workspace has one size).  The
// rounding chain is fixed: N0 = 0.5 (1 - xi), N1 = 0.5 (1 + xi); interpolation axis by axis, x first, as fma(N1, hi, N0 * lo);
// a derivative is 0.5 (hi - lo) on its own axis; the scale s_d multiplies last.  The squares are summed in fp64 per thread, then
// through the fixed-order reduction of dn_reduce.h.
//
// Adjoint: dense over nodes in gather form.  Node (b, k, j, i) visits its at most 2^nsd adjacent elements in the fixed order z, y, x
// (lower neighbour first) and, in each, the element's points in stored order; one fma per term into one fp32 accumulator; one store
// per node.  No atomics: the gradient is bitwise reproducible and independent of the batch a sample sits in.
#include "dn_reduce.h"

namespace dn {

constexpr int PT_THREADS = 256;
constexpr int PT_MAX_BLOCKS = 1024;      // forward workgroups: 256 k points in flight; more points loop
static constexpr int64_t PT_WORKSPACE = DN_WS_HEADER + (int64_t)(2 * sizeof(double)) * PT_MAX_BLOCKS;

struct PtParams {
    const float* u;
    const int32_t* elem;
    const float* xi;
    const int32_t* offsets;
    int npts, total;              // points per sample, points in all
    int nx, ny, nz, nelx, nely, nelz;
    int nodes, nel;               // per sample
    float s[3];
    int kind, penalty;
    const float* target;
    float target_value;
    const float* normals;
    float cv, cn;                 // 2 w_val, 2 w_nrm
    double w_val, w_nrm;
    float* values;
    float* pgrads;
    float* cot_out;
    double* sums;
    unsigned* counter;
    double* part;
    const float* cot;
    const float* gscale_dev;
    float gscale;
    float* grad;
    int accumulate;
};

template <int NSD>
__global__ void __launch_bounds__(PT_THREADS) points_forward_kernel(const PtParams p) {
    __shared__ double red[2 * PT_THREADS / DN_WAVE];
    __shared__ int last_flag;
    const int tid = threadIdx.x;
    const size_t T = (size_t)p.total;
    double sv = 0.0, sn = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * PT_THREADS + tid; q < p.total; q += (int64_t)gridDim.x * PT_THREADS) {
        const int b = (int)(q / p.npts);
        const int e = min(max(p.elem[q], 0), p.nel - 1);
        const int ex = e % p.nelx, er = e / p.nelx;
        const int ey = NSD == 3 ? er % p.nely : er, ez = NSD == 3 ? er / p.nely : 0;
        const float* ub = p.u + (size_t)b * (size_t)p.nodes + ((size_t)ez * p.ny + ey) * (size_t)p.nx + ex;
        const float xx = p.xi[q], xy = p.xi[T + q];
        const float nx0 = 0.5f * (1.f - xx), nx1 = 0.5f * (1.f + xx);
        const float ny0 = 0.5f * (1.f - xy), ny1 = 0.5f * (1.f + xy);
        float val, g[3] = {0.f, 0.f, 0.f};
        float bv[2], bx[2], by[2];                     // per z level: value, d/dx, d/dy after the x and y passes
#pragma unroll
        for (int k = 0; k < (NSD == 3 ? 2 : 1); ++k) {
            const float* uk = ub + (size_t)k * p.ny * (size_t)p.nx;
            const float u00 = uk[0], u10 = uk[1], u01 = uk[p.nx], u11 = uk[p.nx + 1];
            const float a0 = fmaf(nx1, u10, nx0 * u00), a1 = fmaf(nx1, u11, nx0 * u01);
            const float d0 = 0.5f * (u10 - u00), d1 = 0.5f * (u11 - u01);
            bv[k] = fmaf(ny1, a1, ny0 * a0);
            bx[k] = fmaf(ny1, d1, ny0 * d0);
            by[k] = 0.5f * (a1 - a0);
        }
        if constexpr (NSD == 3) {
            const float xz = p.xi[2 * T + q];
            const float nz0 = 0.5f * (1.f - xz), nz1 = 0.5f * (1.f + xz);
            val = fmaf(nz1, bv[1], nz0 * bv[0]);
            g[0] = p.s[0] * fmaf(nz1, bx[1], nz0 * bx[0]);
            g[1] = p.s[1] * fmaf(nz1, by[1], nz0 * by[0]);
            g[2] = p.s[2] * (0.5f * (bv[1] - bv[0]));
        } else {
            val = bv[0];
            g[0] = p.s[0] * bx[0];
            g[1] = p.s[1] * by[0];
        }
        if (p.values) p.values[q] = val;
        if (p.pgrads) {
#pragma unroll
            for (int d = 0; d < NSD; ++d) p.pgrads[(size_t)d * T + q] = g[d];
        }
        if (p.penalty) {
            const float dv = val - (p.target ? p.target[q] : p.target_value);
            sv = fma((double)dv, (double)dv, sv);
            float c[3] = {0.f, 0.f, 0.f};
            if (p.kind != DN_POINTS_NONE) {
                float n[3];
#pragma unroll
                for (int d = 0; d < NSD; ++d) n[d] = p.normals[(size_t)d * T + q];
                if (p.kind == DN_POINTS_DOT) {
                    float dot = g[0] * n[0];
#pragma unroll
                    for (int d = 1; d < NSD; ++d) dot = fmaf(g[d], n[d], dot);
                    const float r = dot - 1.f;
                    sn = fma((double)r, (double)r, sn);
                    const float cr = p.cn * r;
#pragma unroll
                    for (int d = 0; d < NSD; ++d) c[d] = cr * n[d];
                } else {
#pragma unroll
                    for (int d = 0; d < NSD; ++d) {
                        const float r = g[d] - n[d];
                        sn = fma((double)r, (double)r, sn);
                        c[d] = p.cn * r;
                    }
                }
            }
            if (p.cot_out) {
                p.cot_out[q] = p.cv * dv;
#pragma unroll
                for (int d = 0; d < NSD; ++d) p.cot_out[(size_t)(1 + d) * T + q] = c[d];
            }
        }
    }
    if (!p.sums) return;                                    // (wave-uniform: a kernel argument)
    block_sum2(sv, sn, red, tid, PT_THREADS);
    const int nblocks = launch_workgroups();
    double* parts[2] = {p.part, p.part + nblocks};
    const double mine[2] = {sv, sn};
    double tot[2];
    if (!last_arriver_sums<2, 8, true, true>(parts, p.counter, mine, tid, PT_THREADS, &last_flag, tot)) return;
    block_sum2(tot[0], tot[1], red, tid, PT_THREADS);
    if (tid == 0) {
        const double a = p.w_val * tot[0], c = p.w_nrm * tot[1];
        p.sums[0] = a;
        p.sums[1] = c;
        p.sums[2] = a + c;
        arrival_reset(p.counter);
        p.counter[DN_WS_TICKET_WORD] = 0u;
    }
}

// The points q0 <= q < q1 of one element, seen from its node with the 1-D weights / derivative signs below:
//   acc += c0 N_a + sum_d c_d (s_d d_d N_a),   N_a = wx wy [wz],   wx = 0.5 (1 + sx xi_x)  (sx = -1: the element's lower node in x)
template <int NSD>
__device__ __forceinline__ float pt_gather(const PtParams& p, int q0, int q1, float sx, float sy, float sz, float acc) {
    const size_t T = (size_t)p.total;
    const float hx = 0.5f * sx * p.s[0], hy = 0.5f * sy * p.s[1], hz = 0.5f * sz * p.s[2];      // exact: +-0.5 s_d
    for (int q = q0; q < q1; ++q) {
        const float wx = 0.5f * fmaf(sx, p.xi[q], 1.f), wy = 0.5f * fmaf(sy, p.xi[T + q], 1.f);
        const float c0 = p.cot[q], cx = p.cot[T + q], cy = p.cot[2 * T + q];
        if constexpr (NSD == 3) {
            const float wz = 0.5f * fmaf(sz, p.xi[2 * T + q], 1.f);
            const float cz = p.cot[3 * T + q];
            const float wxy = wx * wy;
            acc = fmaf(c0, wxy * wz, acc);
            acc = fmaf(cx, hx * (wy * wz), acc);
            acc = fmaf(cy, hy * (wx * wz), acc);
            acc = fmaf(cz, hz * wxy, acc);
        } else {
            acc = fmaf(c0, wx * wy, acc);
            acc = fmaf(cx, hx * wy, acc);
            acc = fmaf(cy, hy * wx, acc);
        }
    }
    return acc;
}

template <int NSD>
__global__ void __launch_bounds__(PT_THREADS) points_adjoint_kernel(const PtParams p) {
    const int n = blockIdx.x * PT_THREADS + threadIdx.x;      // node within the sample, x fastest
    if (n >= p.nodes) return;
    const int b = blockIdx.y;
    const int i = n % p.nx, r = n / p.nx;
    const int j = NSD == 3 ? r % p.ny : r, k = NSD == 3 ? r / p.ny : 0;
    const int32_t* off = p.offsets + (size_t)b * (size_t)p.nel;
    const int first = b * p.npts, end = first + p.npts;        // the sample's own range of the sorted list
    float acc = 0.f;
    int seen = 0;
#pragma unroll
    for (int dk = (NSD == 3 ? -1 : 0); dk <= 0; ++dk) {
        const int ez = k + dk;
        if (NSD == 3 && (ez < 0 || ez >= p.nelz)) continue;
#pragma unroll
        for (int dj = -1; dj <= 0; ++dj) {
            const int ey = j + dj;
            if (ey < 0 || ey >= p.nely) continue;
            // one row of elements: the points of element i - 1 end where those of element i begin
            const int row = (ez * p.nely + ey) * p.nelx;
            int lo = off[row + max(i - 1, 0)], mid = off[row + min(i, p.nelx)], hi = off[row + min(i + 1, p.nelx)];
            lo = min(max(lo, first), end);
            mid = min(max(mid, lo), end);
            hi = min(max(hi, mid), end);
            const float sy = dj ? 1.f : -1.f, sz = dk ? 1.f : -1.f;
            acc = pt_gather<NSD>(p, lo, mid, 1.f, sy, sz, acc);
            acc = pt_gather<NSD>(p, mid, hi, -1.f, sy, sz, acc);
            seen += hi - lo;
        }
    }
    float gs = p.gscale;
    if (p.gscale_dev) gs *= p.gscale_dev[0];
    float* gp = p.grad + (size_t)b * (size_t)p.nodes + n;
    const float v = __fmul_rn(gs, acc);                        // rounded on its own: accumulate adds the same bits a plain store writes
    if (p.accumulate) {
        if (seen) *gp = __fadd_rn(*gp, v);                     // a node no point touches keeps its bits (-0 included)
    } else {
        *gp = v;
    }
}

static inline int pt_validate_mesh(const dn_mesh* m) {
    if (!m) return DN_E_BADARG;
    if (m->nsd != 2 && m->nsd != 3) return DN_E_BADARG;
    if (m->batch < 1 || m->batch > 65535 || m->nx < 2 || m->ny < 2 || (m->nsd == 3 ? m->nz < 2 : m->nz != 1)) return DN_E_BADARG;
    if (m->degree != 1) return m->degree == 2 || m->degree == 3 ? DN_E_UNSUPPORTED : DN_E_BADARG;
    if ((int64_t)m->nx * m->ny * m->nz >= (1ll << 30)) return DN_E_UNSUPPORTED;
    return 0;
}

}  // namespace dn

using namespace dn;

extern "C" int64_t dn_points_workspace_bytes(const dn_mesh* mesh) {
    const int rc = pt_validate_mesh(mesh);
    return rc ? rc : PT_WORKSPACE;
}

extern "C" int dn_points_apply(const dn_mesh* mesh, const dn_points_args* a, void* stream) {
    int rc = pt_validate_mesh(mesh);
    if (rc) return rc;
    if (!a) return DN_E_BADARG;
    const int nsd = mesh->nsd, B = mesh->batch;
    if (a->npts < 0 || (int64_t)B * a->npts > 0x7fffffffll) return DN_E_BADARG;
    if (a->kind != DN_POINTS_NONE && a->kind != DN_POINTS_DOT && a->kind != DN_POINTS_MATCH) return DN_E_BADARG;
    if ((a->penalty | a->accumulate) & ~1) return DN_E_BADARG;
    const bool forward = a->values || a->pgrads || a->penalty, adjoint = a->grad != nullptr;
    if (!forward && !adjoint) return DN_E_BADARG;                      // nothing to compute (accumulate without grad included)
    if (a->accumulate && !a->grad) return DN_E_BADARG;
    if (!a->penalty && a->sums) return DN_E_BADARG;
    if (a->penalty && !a->sums && !a->cot) return DN_E_BADARG;         // a penalty nobody reads
    const int total = (int)((int64_t)B * a->npts);
    if (forward && !a->u) return DN_E_BADARG;
    if (total > 0) {
        if (!a->xi) return DN_E_BADARG;
        if (forward && !a->elem) return DN_E_BADARG;
        if (a->penalty && a->kind != DN_POINTS_NONE && !a->normals) return DN_E_BADARG;
        if (adjoint && (!a->offsets || !a->cot)) return DN_E_BADARG;
    }
    if (a->sums && (!a->workspace || a->workspace_bytes < PT_WORKSPACE)) return DN_E_WORKSPACE;

    PtParams p;
    p.u = a->u; p.elem = a->elem; p.xi = a->xi; p.offsets = a->offsets;
    p.npts = (int)a->npts; p.total = total;
    p.nx = mesh->nx; p.ny = mesh->ny; p.nz = mesh->nz;
    p.nelx = p.nx - 1; p.nely = p.ny - 1; p.nelz = nsd == 3 ? p.nz - 1 : 1;
    p.nodes = p.nx * p.ny * p.nz;
    p.nel = p.nelx * p.nely * p.nelz;
    for (int d = 0; d < 3; ++d) p.s[d] = d < nsd ? a->dscale[d] : 0.f;
    p.kind = a->kind; p.penalty = a->penalty;
    p.target = a->target; p.target_value = a->target_value; p.normals = a->normals;
    p.cv = 2.f * a->w_val; p.cn = 2.f * a->w_nrm;
    p.w_val = (double)a->w_val; p.w_nrm = (double)a->w_nrm;
    p.values = a->values; p.pgrads = a->pgrads; p.cot_out = a->penalty ? a->cot : nullptr;
    p.sums = a->sums;
    p.counter = reinterpret_cast<unsigned*>(a->workspace);
    p.part = a->workspace ? reinterpret_cast<double*>(reinterpret_cast<char*>(a->workspace) + DN_WS_HEADER) : nullptr;
    p.cot = a->cot; p.gscale_dev = a->gscale_dev; p.gscale = a->gscale;
    p.grad = a->grad; p.accumulate = a->accumulate;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (forward && (total > 0 || a->sums)) {                             // no points: one workgroup writes the zero sums
        const int blocks = std::max(1, std::min((total + PT_THREADS - 1) / PT_THREADS, PT_MAX_BLOCKS));
        if (nsd == 3) hipLaunchKernelGGL(points_forward_kernel<3>, dim3(blocks), dim3(PT_THREADS), 0, s, p);
        else hipLaunchKernelGGL(points_forward_kernel<2>, dim3(blocks), dim3(PT_THREADS), 0, s, p);
        DN_LAUNCH_CHECK();
    }
    if (adjoint && total == 0) {                                         // no points: zeros, or grad left as it is
        if (!a->accumulate) {
            const hipError_t e = hipMemsetAsync(a->grad, 0, sizeof(float) * (size_t)B * (size_t)p.nodes, s);
            if (e != hipSuccess) return (int)e;
        }
    } else if (adjoint) {
        const dim3 grid((p.nodes + PT_THREADS - 1) / PT_THREADS, B);
        if (nsd == 3) hipLaunchKernelGGL(points_adjoint_kernel<3>, grid, dim3(PT_THREADS), 0, s, p);
        else hipLaunchKernelGGL(points_adjoint_kernel<2>, grid, dim3(PT_THREADS), 0, s, p);
        DN_LAUNCH_CHECK();
    }
    return 0;
}
