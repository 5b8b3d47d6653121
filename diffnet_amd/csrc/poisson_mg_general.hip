// The grid transfers of a multigrid V-cycle between Q1 meshes that need NOT be nested: dn_poisson_mg_transfer (include/diffnet_hip.h).
// The coarse mesh of an axis with e elements has ceil(e / 2) elements over the same length, so a coarse node in general sits between
// two fine nodes; where e is even the axis is nested and this kernel does on it what csrc/poisson_mg.hip does.  The per-axis
// interpolation P (fine node i <- coarse nodes j, j + 1 with two weights) is NOT computed here: the host rounds every weight once to
// float32 and hands over two views of the same numbers per axis,
//     parents[d][i]  = { j, w0, w1 }                    a row of the 1-D P: what PROLONG reads,
//     children[d][j] = { first, count, w[4] }           a column of it: the fine nodes first .. first + count - 1 that have coarse node j
//                                                       as a parent, and their weights on it: what RESTRICT reads,
// so RESTRICT is the transpose of PROLONG as float32 matrices whatever a float division would round to here.  A coarse node has at
// most 4 children per axis (the open interval of fine coordinates between its two coarse neighbours is at most 4 fine spacings long).
//     RESTRICT  c = Z_c P^T (b - q)   one thread per COARSE node gathers its count_z x count_y x 4 fine nodes, rows added in the fixed
//               order z, y, x; the x entries beyond count_x are selected away, rows beyond count_y / count_z are skipped.  The fine
//               residual b - q is formed in registers and never written.
//     PROLONG   x += Z_f P c          one thread per FINE node reads its 2^nsd parents, one code path for every node.
// Thread mapping as in poisson_mg.hip: a flat index within the sample, 256 threads a workgroup, x fastest; the written side (and the
// fine side of PROLONG's update) is one contiguous dword per lane.  The roughly-stride-2 side: RESTRICT's four loads of a fine row each
// take about every second dword of the ~512 bytes the wave spans -- the lines come into the L1 once and serve four instructions (three
// in the nested kernel), so HBM and L2 see a contiguous read and the cost is load instructions: up to 2 x 16 of them per coarse node
// in 2-D and 2 x 64 in 3-D, against 2 x 9 and 2 x 27 nested.  PROLONG's coarse loads have about two lanes per dword.  The tables are a
// few KiB, indexed by the node's own coordinates, and stay in the caches; a thread reads one 16-byte entry per axis (two in RESTRICT).
// Indices read from a table are clamped into the mesh before they address anything.
// Every output node is written by exactly one thread with additions in an order that depends on the node alone; no atomics, no
// workspace: bitwise reproducible and independent of the batch size.
#include "dn_common.h"

namespace dn {

constexpr int MGT_THREADS = 256;

struct MgtParams {
    float* x;
    const float* b;
    const float* q;
    float* c;
    const uint8_t* mask;
    int mask_batched;
    int fx, fy, fz, cx, cy, cz;
    unsigned nf, nc;
    const dn_mg_parent* parents[3];
    const dn_mg_children* children[3];
};

__device__ __forceinline__ dn_mg_children mgt_children(const dn_mg_children* t, int j) {
    const int4 h = *reinterpret_cast<const int4*>(t + j);
    const float4 w = *reinterpret_cast<const float4*>(t[j].w);
    dn_mg_children r;
    r.first = h.x; r.count = h.y; r.pad[0] = r.pad[1] = 0;
    r.w[0] = w.x; r.w[1] = w.y; r.w[2] = w.z; r.w[3] = w.w;
    return r;
}

template <int NSD>
__global__ void __launch_bounds__(MGT_THREADS) mgt_restrict_kernel(const MgtParams p) {
    const unsigned idx = blockIdx.x * MGT_THREADS + threadIdx.x;
    if (idx >= p.nc) return;
    const int b = blockIdx.y;
    const int ic = (int)(idx % (unsigned)p.cx);
    const unsigned t = idx / (unsigned)p.cx;
    const int jc = (int)(t % (unsigned)p.cy), kc = (int)(t / (unsigned)p.cy);
    const float* bb = p.b + (int64_t)b * p.nf;
    const float* qb = p.q + (int64_t)b * p.nf;
    const dn_mg_children X = mgt_children(p.children[0], ic), Y = mgt_children(p.children[1], jc);
    dn_mg_children Z;
    Z.first = 0; Z.count = 1; Z.w[0] = 1.f; Z.w[1] = Z.w[2] = Z.w[3] = 0.f;
    if constexpr (NSD == 3) Z = mgt_children(p.children[2], kc);
    // clamped into the mesh: an entry beyond `count` is selected away or skipped
    const int x0 = min(max(X.first, 0), p.fx - 1), y0 = min(max(Y.first, 0), p.fy - 1), z0 = min(max(Z.first, 0), p.fz - 1);
    unsigned xo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) xo[e] = (unsigned)min(x0 + e, p.fx - 1);
    float acc = 0.f;
#pragma unroll
    for (int dz = 0; dz < (NSD == 3 ? 4 : 1); ++dz) {
        if (dz >= Z.count) continue;
        const unsigned k = (unsigned)min(z0 + dz, p.fz - 1);
        float plane = 0.f;
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            if (dy >= Y.count) continue;
            const unsigned row = (k * (unsigned)p.fy + (unsigned)min(y0 + dy, p.fy - 1)) * (unsigned)p.fx;
            float r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = bb[row + xo[e]] - qb[row + xo[e]];
            float rowsum = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) rowsum += e < X.count ? X.w[e] * r[e] : 0.f;
            plane += Y.w[dy] * rowsum;
        }
        acc += Z.w[dz] * plane;
    }
    const bool fixed = p.mask && p.mask[(p.mask_batched ? (int64_t)b * p.nc : 0) + idx] != 0;
    p.c[(int64_t)b * p.nc + idx] = fixed ? 0.f : acc;
}

template <int NSD>
__global__ void __launch_bounds__(MGT_THREADS) mgt_prolong_kernel(const MgtParams p) {
    const unsigned idx = blockIdx.x * MGT_THREADS + threadIdx.x;
    if (idx >= p.nf) return;
    const int b = blockIdx.y;
    if (p.mask && p.mask[(p.mask_batched ? (int64_t)b * p.nf : 0) + idx] != 0) return;       // Z_f: a Dirichlet node keeps its value
    const int i = (int)(idx % (unsigned)p.fx);
    const unsigned t = idx / (unsigned)p.fx;
    const int j = (int)(t % (unsigned)p.fy), k = (int)(t / (unsigned)p.fy);
    const float* cb = p.c + (int64_t)b * p.nc;
    const float4 X = *reinterpret_cast<const float4*>(p.parents[0] + i), Y = *reinterpret_cast<const float4*>(p.parents[1] + j);
    // the parents j, j + 1 clamped into the coarse mesh (it has at least 3 nodes per axis)
    const unsigned i0 = (unsigned)min(max(__float_as_int(X.x), 0), p.cx - 2), j0 = (unsigned)min(max(__float_as_int(Y.x), 0), p.cy - 2);
    auto plane = [&](unsigned kk) {
        const unsigned r0 = (kk * (unsigned)p.cy + j0) * (unsigned)p.cx + i0, r1 = r0 + (unsigned)p.cx;
        return Y.y * (X.y * cb[r0] + X.z * cb[r0 + 1]) + Y.z * (X.y * cb[r1] + X.z * cb[r1 + 1]);
    };
    float e;
    if constexpr (NSD == 3) {
        const float4 Z = *reinterpret_cast<const float4*>(p.parents[2] + k);
        const unsigned k0 = (unsigned)min(max(__float_as_int(Z.x), 0), p.cz - 2);
        e = Z.y * plane(k0) + Z.z * plane(k0 + 1);
    } else {
        e = plane(0u);
    }
    float* xb = p.x + (int64_t)b * p.nf;
    xb[idx] += e;
}

}  // namespace dn

using namespace dn;

static_assert(sizeof(dn_mg_parent) == 16 && sizeof(dn_mg_children) == 32, "the table entries are read as 16-byte vectors");

extern "C" int dn_poisson_mg_transfer(const dn_poisson_mg_transfer_args* a, void* stream) {
    if (!a) return DN_E_BADARG;
    const int op = a->op;
    if (op != DN_MG_RESTRICT && op != DN_MG_PROLONG) return DN_E_BADARG;
    if (a->nsd != 2 && a->nsd != 3) return DN_E_BADARG;
    if (a->batch < 1 || a->batch > 65535) return DN_E_BADARG;
    int f[3] = {1, 1, 1}, c[3] = {1, 1, 1};
    for (int d = 0; d < a->nsd; ++d) {
        f[d] = a->fine[d];
        c[d] = a->coarse[d];
        // at least 3 elements on the fine axis, ceil(e / 2) on the coarse one
        if (f[d] < 4 || c[d] != f[d] / 2 + 1) return DN_E_BADARG;
        if (!a->parents[d] || !a->children[d]) return DN_E_BADARG;
        if ((reinterpret_cast<uintptr_t>(a->parents[d]) | reinterpret_cast<uintptr_t>(a->children[d])) & 15) return DN_E_BADARG;
    }
    const int64_t nf = (int64_t)f[0] * f[1] * f[2], nc = (int64_t)c[0] * c[1] * c[2];
    if (nf >= (1ll << 30)) return DN_E_BADARG;
    if (a->mask_batched & ~1) return DN_E_BADARG;
    if (op == DN_MG_RESTRICT && (!a->b || !a->q || !a->c)) return DN_E_BADARG;
    if (op == DN_MG_PROLONG && (!a->x || !a->c)) return DN_E_BADARG;
    for (const void* q : {(const void*)a->x, (const void*)a->b, (const void*)a->q, (const void*)a->c})
        if (reinterpret_cast<uintptr_t>(q) & 15) return DN_E_BADARG;

    MgtParams pp = {};
    pp.x = a->x; pp.b = a->b; pp.q = a->q; pp.c = a->c;
    pp.mask = a->mask; pp.mask_batched = a->mask_batched;
    pp.fx = f[0]; pp.fy = f[1]; pp.fz = f[2]; pp.cx = c[0]; pp.cy = c[1]; pp.cz = c[2];
    pp.nf = (unsigned)nf; pp.nc = (unsigned)nc;
    for (int d = 0; d < 3; ++d) {
        pp.parents[d] = d < a->nsd ? a->parents[d] : nullptr;
        pp.children[d] = d < a->nsd ? a->children[d] : nullptr;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 block(MGT_THREADS);
    const auto blocks = [](int64_t items) { return (unsigned)((items + MGT_THREADS - 1) / MGT_THREADS); };
    if (op == DN_MG_RESTRICT) {
        const dim3 grid(blocks(nc), a->batch);
        if (a->nsd == 2) hipLaunchKernelGGL(mgt_restrict_kernel<2>, grid, block, 0, s, pp);
        else hipLaunchKernelGGL(mgt_restrict_kernel<3>, grid, block, 0, s, pp);
    } else {
        const dim3 grid(blocks(nf), a->batch);
        if (a->nsd == 2) hipLaunchKernelGGL(mgt_prolong_kernel<2>, grid, block, 0, s, pp);
        else hipLaunchKernelGGL(mgt_prolong_kernel<3>, grid, block, 0, s, pp);
    }
    DN_LAUNCH_CHECK();
    return 0;
}
