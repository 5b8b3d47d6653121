// The grid transfers and the smoother update of a geometric multigrid V-cycle on nested Q1 meshes: dn_poisson_mg
// (include/diffnet_hip.h).  The V-cycle is the preconditioner z = M r of the batched CG solve (diffnet_amd/solve.py, dn_poisson_pcg in
// csrc/poisson_cg.hip); a level's operator is dn_poisson_apply on that level's mesh and its inverse diagonal dn_poisson_diag, so what a
// cycle lacked is below.  The coarse mesh has (n - 1) / 2 + 1 nodes per axis, coarse node i sits on fine node 2 i.
//     RESTRICT  c = Z_c P^T (b - q)   one thread per COARSE node gathers the 3^nsd fine nodes around fine node 2 i with the per-axis
//               weights 1/2, 1, 1/2 (exact in float32), rows added in the fixed order z, y, x; a neighbour beyond a face is absent.
//               The fine residual b - q is formed in registers and never written.
//     PROLONG   x += Z_f P c          one thread per FINE node averages the 2^nsd coarse nodes (i >> 1, (i + 1) >> 1 per axis; on an
//               even index the two coincide and the average is exact), one code path for every parity, and adds it to x.
//     SMOOTH    x += omega dinv (b - q),  SMOOTH0  x = omega dinv b        16 bytes per lane, the quads of poisson_cg.hip.
// All four are bandwidth-bound.  Thread mapping: a flat index within the sample, 256 threads a workgroup, x fastest.  The side of a
// transfer that is WRITTEN (and the fine side of PROLONG's update) is one dword per lane, contiguous across the wave.  The stride-2 side
// is where coalescing is lost: RESTRICT's three loads of a fine row each take every second dword of the 512 bytes the wave spans, so each
// line is fetched into the L1 once and used by three instructions -- the HBM and L2 traffic is that of a contiguous read, the cost is
// three times the load instructions; PROLONG's coarse loads have two lanes per dword (a broadcast within the line).  Both read every
// byte of their level exactly once from L2's point of view.  On the small levels of a cycle these launches are launch-bound, not
// bandwidth-bound (profiles/poisson_multigrid.txt).
// Every output node is written by exactly one thread with additions in an order that depends on the node alone; no atomics, no
// workspace: bitwise reproducible and independent of the batch size.  A sample's base is only 4-byte aligned when n is odd (it always is
// on a transfer's levels): SMOOTH's quads are 4-byte-aligned dwordx4 accesses as in poisson_cg.hip.
#include "dn_common.h"

namespace dn {

struct __attribute__((packed, aligned(4))) MgF4 { float v[4]; };

constexpr int MG_THREADS = 256;

struct MgParams {
    float* x;
    const float* b;
    const float* q;
    const float* dinv;
    float* c;
    const uint8_t* mask;
    int dinv_batched, mask_batched;
    int fx, fy, fz, cx, cy, cz;
    unsigned nf, nc;
    float omega;
};

template <int NSD>
__global__ void __launch_bounds__(MG_THREADS) mg_restrict_kernel(const MgParams p) {
    const unsigned idx = blockIdx.x * MG_THREADS + threadIdx.x;
    if (idx >= p.nc) return;
    const int b = blockIdx.y;
    const int ic = (int)(idx % (unsigned)p.cx);
    const unsigned t = idx / (unsigned)p.cx;
    const int jc = (int)(t % (unsigned)p.cy), kc = (int)(t / (unsigned)p.cy);
    const float* bb = p.b + (int64_t)b * p.nf;
    const float* qb = p.q + (int64_t)b * p.nf;
    const int fi = 2 * ic, fj = 2 * jc, fk = 2 * kc;
    constexpr int Z0 = NSD == 3 ? -1 : 0, Z1 = NSD == 3 ? 1 : 0;
    const bool xl = fi > 0, xr = fi < p.fx - 1;
    float acc = 0.f;
#pragma unroll
    for (int dz = Z0; dz <= Z1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int k = fk + dz, j = fj + dy;
            const bool in = j >= 0 && j < p.fy && k >= 0 && k < p.fz;
            // indices clamped into the mesh: a clamped value is multiplied by a zero weight
            const unsigned row = ((unsigned)min(max(k, 0), p.fz - 1) * (unsigned)p.fy + (unsigned)min(max(j, 0), p.fy - 1)) * (unsigned)p.fx;
            const unsigned o0 = row + (unsigned)max(fi - 1, 0), o1 = row + (unsigned)fi, o2 = row + (unsigned)min(fi + 1, p.fx - 1);
            const float l = bb[o0] - qb[o0], m = bb[o1] - qb[o1], r = bb[o2] - qb[o2];
            const float rowsum = (xl ? 0.5f * l : 0.f) + m + (xr ? 0.5f * r : 0.f);
            const float w = (dy == 0 ? 1.f : 0.5f) * (dz == 0 ? 1.f : 0.5f);
            acc += in ? w * rowsum : 0.f;
        }
    const bool fixed = p.mask && p.mask[(p.mask_batched ? (int64_t)b * p.nc : 0) + idx] != 0;
    p.c[(int64_t)b * p.nc + idx] = fixed ? 0.f : acc;
}

template <int NSD>
__global__ void __launch_bounds__(MG_THREADS) mg_prolong_kernel(const MgParams p) {
    const unsigned idx = blockIdx.x * MG_THREADS + threadIdx.x;
    if (idx >= p.nf) return;
    const int b = blockIdx.y;
    if (p.mask && p.mask[(p.mask_batched ? (int64_t)b * p.nf : 0) + idx] != 0) return;       // Z_f: a Dirichlet node keeps its value
    const int i = (int)(idx % (unsigned)p.fx);
    const unsigned t = idx / (unsigned)p.fx;
    const int j = (int)(t % (unsigned)p.fy), k = (int)(t / (unsigned)p.fy);
    const float* cb = p.c + (int64_t)b * p.nc;
    const unsigned i0 = (unsigned)(i >> 1), i1 = (unsigned)((i + 1) >> 1);
    const unsigned j0 = (unsigned)(j >> 1), j1 = (unsigned)((j + 1) >> 1);
    auto plane = [&](unsigned kk) {
        const unsigned r0 = (kk * (unsigned)p.cy + j0) * (unsigned)p.cx, r1 = (kk * (unsigned)p.cy + j1) * (unsigned)p.cx;
        return (cb[r0 + i0] + cb[r0 + i1]) + (cb[r1 + i0] + cb[r1 + i1]);
    };
    float e;
    if constexpr (NSD == 3) e = 0.125f * (plane((unsigned)(k >> 1)) + plane((unsigned)((k + 1) >> 1)));
    else e = 0.25f * plane(0u);
    float* xb = p.x + (int64_t)b * p.nf;
    xb[idx] += e;
}

template <bool FIRST>
__global__ void __launch_bounds__(MG_THREADS) mg_smooth_kernel(const MgParams p) {
    const int b = blockIdx.y;
    const int64_t base = (int64_t)b * p.nf;
    float* xb = p.x + base;
    const float* bb = p.b + base;
    const float* qb = FIRST ? nullptr : p.q + base;
    const float* db = p.dinv + (p.dinv_batched ? base : 0);
    const float om = p.omega;
    const unsigned i = (blockIdx.x * MG_THREADS + threadIdx.x) * 4u;
    if (i >= p.nf) return;
    if (i + 4u <= p.nf) {
        const MgF4 bv = *reinterpret_cast<const MgF4*>(bb + i), dv = *reinterpret_cast<const MgF4*>(db + i);
        MgF4 xv;
        if constexpr (FIRST) {
#pragma unroll
            for (int c = 0; c < 4; ++c) xv.v[c] = om * dv.v[c] * bv.v[c];
        } else {
            const MgF4 qv = *reinterpret_cast<const MgF4*>(qb + i);
            xv = *reinterpret_cast<const MgF4*>(xb + i);
#pragma unroll
            for (int c = 0; c < 4; ++c) xv.v[c] = fmaf(om * dv.v[c], bv.v[c] - qv.v[c], xv.v[c]);
        }
        *reinterpret_cast<MgF4*>(xb + i) = xv;
    } else {
        for (unsigned e = i; e < p.nf; ++e) {                 // the last < 4 nodes of the sample
            if constexpr (FIRST) xb[e] = om * db[e] * bb[e];
            else xb[e] = fmaf(om * db[e], bb[e] - qb[e], xb[e]);
        }
    }
}

}  // namespace dn

using namespace dn;

extern "C" int dn_poisson_mg(const dn_poisson_mg_args* a, void* stream) {
    if (!a) return DN_E_BADARG;
    const int op = a->op;
    if (op < DN_MG_RESTRICT || op > DN_MG_SMOOTH0) return DN_E_BADARG;
    if (a->nsd != 2 && a->nsd != 3) return DN_E_BADARG;
    if (a->batch < 1 || a->batch > 65535) return DN_E_BADARG;
    const bool transfer = op == DN_MG_RESTRICT || op == DN_MG_PROLONG;
    int f[3], c[3];
    for (int d = 0; d < 3; ++d) {
        f[d] = d < a->nsd ? a->fine[d] : 1;
        c[d] = d < a->nsd ? a->coarse[d] : 1;
        if (d >= a->nsd) continue;
        if (f[d] < 2) return DN_E_BADARG;
        if (transfer && (f[d] < 3 || !(f[d] & 1) || c[d] != (f[d] - 1) / 2 + 1)) return DN_E_BADARG;
    }
    const int64_t nf = (int64_t)f[0] * f[1] * f[2], nc = (int64_t)c[0] * c[1] * c[2];
    if (nf >= (1ll << 30)) return DN_E_UNSUPPORTED;
    if ((a->dinv_batched | a->mask_batched) & ~1) return DN_E_BADARG;
    if (!(a->omega == a->omega)) return DN_E_BADARG;
    if (op == DN_MG_RESTRICT && (!a->b || !a->q || !a->c)) return DN_E_BADARG;
    if (op == DN_MG_PROLONG && (!a->x || !a->c)) return DN_E_BADARG;
    if (op == DN_MG_SMOOTH && (!a->x || !a->b || !a->q || !a->dinv)) return DN_E_BADARG;
    if (op == DN_MG_SMOOTH0 && (!a->x || !a->b || !a->dinv)) return DN_E_BADARG;
    for (const void* q : {(const void*)a->x, (const void*)a->b, (const void*)a->q, (const void*)a->dinv, (const void*)a->c})
        if (reinterpret_cast<uintptr_t>(q) & 15) return DN_E_BADARG;

    MgParams pp = {};
    pp.x = a->x; pp.b = a->b; pp.q = a->q; pp.dinv = a->dinv; pp.c = a->c;
    pp.mask = transfer ? a->mask : nullptr;
    pp.dinv_batched = a->dinv_batched; pp.mask_batched = a->mask_batched;
    pp.fx = f[0]; pp.fy = f[1]; pp.fz = f[2]; pp.cx = c[0]; pp.cy = c[1]; pp.cz = c[2];
    pp.nf = (unsigned)nf; pp.nc = (unsigned)nc;
    pp.omega = a->omega;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 block(MG_THREADS);
    const auto blocks = [](int64_t items) { return (unsigned)((items + MG_THREADS - 1) / MG_THREADS); };
    if (op == DN_MG_RESTRICT) {
        const dim3 grid(blocks(nc), a->batch);
        if (a->nsd == 2) hipLaunchKernelGGL(mg_restrict_kernel<2>, grid, block, 0, s, pp);
        else hipLaunchKernelGGL(mg_restrict_kernel<3>, grid, block, 0, s, pp);
    } else if (op == DN_MG_PROLONG) {
        const dim3 grid(blocks(nf), a->batch);
        if (a->nsd == 2) hipLaunchKernelGGL(mg_prolong_kernel<2>, grid, block, 0, s, pp);
        else hipLaunchKernelGGL(mg_prolong_kernel<3>, grid, block, 0, s, pp);
    } else {
        const dim3 grid(blocks((nf + 3) / 4), a->batch);
        if (op == DN_MG_SMOOTH) hipLaunchKernelGGL(mg_smooth_kernel<false>, grid, block, 0, s, pp);
        else hipLaunchKernelGGL(mg_smooth_kernel<true>, grid, block, 0, s, pp);
    }
    DN_LAUNCH_CHECK();
    return 0;
}
