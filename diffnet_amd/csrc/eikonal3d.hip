// Fused 3-D stabilised eikonal weak-form residual on structured Q1 meshes and its VJP: dn_eikonal3d_apply (include/diffnet_hip.h).
//
// The domain term of the 3-D eikonal scripts of the reference, examples/eiqonal/single_instance/05_3d_sphere_loss4.py:269-425 (loss4;
// 04_3d_sphere_recon.py::loss is its unstabilised form): the two Dirichlet substitutions, the Gauss-point evaluations of u, u_x, u_y and
// u_z, the stabilised weak form, its assembly, the zeroed Dirichlet rows and the Frobenius norm -- in one launch.
//
//   R_a   = zero_on_dirichlet( sum_{e contains a} sum_g W_g ( N_a A + Nx_a B + Ny_a C + Nz_a D ) ),  W_g = gpw_g wscale
//   A = sq |grad u~|^2 - f      (B, C, D) = tau u~ grad u~
//   sumsq = sum over (b, nodes) of R^2,   norm = sqrt(sumsq)
// The VJP mode has the same flux form: with the cotangent (zero on the Dirichlet nodes) evaluated like a field (L, grad L)
//   A' = tau grad L . grad u~      (B', C', D') = 2 sq L grad u~ + tau u~ grad L
// so both modes share the element.  The VJP reads u and the cotangent, never the forcing.
//
// Mapping: the one-element form of poisson3d_q1w_kernel (poisson3d_q1.inl).  grid = chunks_x * tiles_y * strips_z * B workgroups of
// (TX, TY) threads; thread (tx, ty) owns one element column of the in-plane tile and marches over the element planes of a z-strip.  The
// element is sum-factorised along z: the in-plane stage of a node plane (u, u_x, u_y at the in-plane Gauss points; the cotangent and the
// nodal forcing likewise) is computed once and used by the layer below and the layer above, and the upper-plane half of a layer's
// transposed sums is carried into the next layer, so a finished plane is transposed in-plane once.  Contributions to the nodes shared
// with the right, up and up-right threads go through a double-buffered LDS slot (one LDS-only barrier per plane); tile and strip seams
// are closed by recomputing the overlap column / row / layer.  No atomics on the data path: every node is written once, by its owner,
// with the same additions in the same order under any launch plan and batch size.  sumsq counts every node once (its owner, after its
// value is complete): per node in fp32, per thread in fp64, then the fixed-order fp64 reduction of dn_reduce.h.  Where the registers
// allow it (PF below) the loads of plane k + 2 are requested before the arithmetic of layer k; the finished plane of layer k is stored
// after the next request.
//
// Optional inputs are compile-time forms: MASK (any condition), BCF (any value field), FK (forcing: constant / nodal / at the Gauss
// points; the VJP has FK == 0 only).  12 forms per rule; the 3- and 4-point rules compile in eikonal3d_g3.hip and eikonal3d_g4.hip.
#include <algorithm>
#include <cstdio>

#include "dn_reduce.h"
#include "elem_args.h"

namespace dn {

struct Ek3Params {
    float b1[4];                           // phi_1 at the 1-D Gauss points (phi_0 = 1 - phi_1)
    float wb0[4], wb1[4], wgz[4];          // w[k] phi_0, w[k] phi_1 and w[k] gz at the 1-D Gauss points (products of uniform values are
                                           // formed on the host: in the kernel they would be hoisted into VGPRs, one per Gauss point)
    float wji[4][4];                       // w[j] * w[i] * wscale
    float gx, gy, gz;                      // phi_1' * 2/h per axis
    float tau, sq, sq2, fconst;            // sq2 = 2 sq
    const float* u;
    const float* cot;                      // VJP: the cotangent of R (u: the linearisation point)
    const float* in_num;                   // VJP: cot is scaled by in_num[0] (/ in_den[0])
    const float* in_den;
    const float* f;                        // FK == 1: nodal forcing
    const float* fgp;                      // FK == 2: (B | 1, G, nelz, nely, nelx)
    int f_batched;
    const void* mask[2];
    int mask_kind[2];                      // 0: none, 1: uint8 (!= 0), 2: fp32 (> 0.5)
    int mask_batched[2];
    const float* bcf[2];
    int bcf_batched[2];
    float bcv[2];
    float* out;
    double* sumsq;
    float* norm;
    double* part;                          // [nblocks] partial sums
    unsigned* counter;
    int nx, ny, nz, nelx, nely, nelz, rows_per_strip, want_sums;
    int chunks_x, tiles_y, strips_z;
    int vjp;
};

// In-plane stage of one node plane at the in-plane Gauss points [j: y][i: x]
template <int NGP, bool VJP, bool FN>
struct Ek3Plane {
    float VU[NGP][NGP], VX[NGP], VY[NGP];                                          // u~, u~_x (constant along x), u~_y (constant along y)
    float LU[VJP ? NGP : 1][VJP ? NGP : 1], LX[VJP ? NGP : 1], LY[VJP ? NGP : 1];  // the cotangent likewise
    float VF[FN ? NGP : 1][FN ? NGP : 1];                                          // nodal forcing
    float keep;                                                                    // 0 where the thread's own node is a Dirichlet node
};

// nodal values a0, a1 (row ey: nodes x0, x0 + 1) and c0, c1 (row ey + 1)
template <int NGP>
__device__ __forceinline__ void ek3_stage(const Ek3Params& p, float a0, float a1, float c0, float c1, float (&VU)[NGP][NGP], float (&VX)[NGP],
                                          float (&VY)[NGP]) {
    const float dx0 = a1 - a0, dx1 = c1 - c0, ddx = dx1 - dx0;
#pragma unroll
    for (int j = 0; j < NGP; ++j) VX[j] = p.gx * fmaf(p.b1[j], ddx, dx0);
#pragma unroll
    for (int i = 0; i < NGP; ++i) {
        const float t0 = fmaf(p.b1[i], dx0, a0);
        const float dy = fmaf(p.b1[i], dx1, c0) - t0;
        VY[i] = p.gy * dy;
#pragma unroll
        for (int j = 0; j < NGP; ++j) VU[j][i] = fmaf(p.b1[j], dy, t0);
    }
}

template <int NGP>
__device__ __forceinline__ void ek3_stage_value(const Ek3Params& p, float a0, float a1, float c0, float c1, float (&VU)[NGP][NGP]) {
    const float dx0 = a1 - a0, dx1 = c1 - c0;
#pragma unroll
    for (int i = 0; i < NGP; ++i) {
        const float t0 = fmaf(p.b1[i], dx0, a0);
        const float dy = fmaf(p.b1[i], dx1, c0) - t0;
#pragma unroll
        for (int j = 0; j < NGP; ++j) VU[j][i] = fmaf(p.b1[j], dy, t0);
    }
}

// Waves per SIMD asked of the compiler: 4 at 2 x 2 x 2 points (<= 128 VGPRs), 3 and 2 for the larger rules (<= 168 / 256 VGPRs); one step
// fewer for the forms that spilled there -- the VJP, which carries two fields per plane, and Gauss-point forcing together with
// conditions (at the 4-point rule: with value fields).  profiles/eikonal3d.txt has what every form takes: none has scratch
constexpr int ek3_waves(int ngp, bool mask, bool bcf, int fk, bool vjp) {
    return ngp == 2 ? (vjp ? 3 : 4) : (ngp == 3 ? ((vjp || (mask && fk == 2)) ? 2 : 3) : ((vjp || (bcf && fk == 2)) ? 1 : 2));
}

template <int NGP, bool MASK, bool BCF, int FK, bool VJP>
__global__ void __launch_bounds__(256, ek3_waves(NGP, MASK, BCF, FK, VJP)) eikonal3d_kernel(const Ek3Params p) {
    static_assert(MASK || !BCF, "a value field belongs to a condition");
    static_assert(!VJP || FK == 0, "the VJP does not read the forcing");
    constexpr int G = NGP * NGP * NGP;
    constexpr bool FN = FK == 1;
    // PF: the next plane's loads are in flight during a layer's arithmetic.  The forms with the most raw values per node (the VJP, a
    // forcing field together with conditions) request and consume a plane in one go instead: with the raw plane alive across the layer they spill
    constexpr bool PF = !VJP && !(MASK && FK != 0);
    using Plane = Ek3Plane<NGP, VJP, FN>;
    const int TX = (int)blockDim.x, TY = (int)blockDim.y;
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    const int tid = ty * TX + tx;
    unsigned lid = xcd_remap(blockIdx.x, gridDim.x);      // logical order chunk, tile, strip, sample: neighbours share their halo in one L2
    const int chunk = (int)(lid % (unsigned)p.chunks_x);
    lid /= (unsigned)p.chunks_x;
    const int tile = (int)(lid % (unsigned)p.tiles_y);
    lid /= (unsigned)p.tiles_y;
    const int strip = (int)(lid % (unsigned)p.strips_z), b = (int)(lid / (unsigned)p.strips_z);
    const int x0 = chunk * (TX - 1) + tx;            // the thread's element column and the node column it owns
    const int ey = tile * (TY - 1) + ty;
    const bool owner = !(chunk > 0 && tx == 0) && !(tile > 0 && ty == 0) && x0 < p.nx && ey < p.ny;
    const bool elem_ok = x0 < p.nelx && ey < p.nely;  // threads beyond the mesh compute on clamped data; their results are dropped
    const unsigned npl = (unsigned)(p.nx * p.ny);
    const int64_t nps = (int64_t)npl * p.nz;
    const unsigned epl = (unsigned)(p.nelx * p.nely);
    const unsigned eps = epl * (unsigned)p.nelz;
    const int R = p.rows_per_strip;
    const int ez_own = strip * R;
    const int ez_begin = ez_own > 0 ? ez_own - 1 : 0;        // the layer under the strip's first node plane is recomputed
    const int ez_end = min(ez_own + R, p.nelz);

    const float* ub = p.u + (int64_t)b * nps;
    const float* lb = VJP ? p.cot + (int64_t)b * nps : ub;
    const float* fb = FK == 1 ? p.f + (p.f_batched ? (int64_t)b * nps : 0) : ub;
    const float* fgb = FK == 2 ? p.fgp + (p.f_batched ? (int64_t)b * G * eps : 0) : ub;
    float* ob = p.out ? p.out + (int64_t)b * nps : nullptr;
    const float* bcfb[2];
    const float* mfp[2];
    const uint8_t* mbp[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        bcfb[k] = p.bcf[k] ? p.bcf[k] + (p.bcf_batched[k] ? (int64_t)b * nps : 0) : ub;
        const int64_t mo = p.mask_batched[k] ? (int64_t)b * nps : 0;
        mfp[k] = p.mask_kind[k] == 2 ? reinterpret_cast<const float*>(p.mask[k]) + mo : ub;
        mbp[k] = p.mask_kind[k] == 1 ? reinterpret_cast<const uint8_t*>(p.mask[k]) + mo : reinterpret_cast<const uint8_t*>(ub);
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

    __shared__ float xch[2][3][256];        // [parity][right | up | up-right][thread]
    __shared__ double red[8];
    __shared__ int last_flag;

    // offsets of the thread's 2 x 2 nodes inside a plane (clamped into the mesh), of its element inside an element plane
    const unsigned row[2] = {(unsigned)min(ey, p.ny - 1) * (unsigned)p.nx, (unsigned)min(ey + 1, p.ny - 1) * (unsigned)p.nx};
    const unsigned col[2] = {(unsigned)min(x0, p.nx - 1), (unsigned)min(x0 + 1, p.nx - 1)};
    const unsigned eoff = (unsigned)min(ey, p.nely - 1) * (unsigned)p.nelx + (unsigned)min(x0, p.nelx - 1);

    struct Raw {
        float u[2][2], l[VJP ? 2 : 1][2], f[FN ? 2 : 1][2];
        float bf[BCF ? 2 : 1][2][2];
        float mf[MASK ? 2 : 1][2][2];          // mask values read as fp32 and as a byte: see plane_issue
        uint8_t mb[MASK ? 2 : 1][2][2];
    };
    auto plane_issue = [&](int zreq, Raw& w) {
        const unsigned zoff = (unsigned)min(zreq, p.nz - 1) * npl;
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const unsigned o = zoff + row[jb] + col[n];
                w.u[jb][n] = ld_at<float>(ub, o);
                if constexpr (VJP) w.l[jb][n] = ld_at<float>(lb, o);
                if constexpr (FN) w.f[jb][n] = ld_at<float>(fb, o);
                // Unconditional loads: a load inside a (uniform) branch makes the compiler wait for every outstanding load at the end
                // of the branch, which serialises the plane's requests.  A condition is read as fp32 AND as a byte, each from its own
                // pointer; the pointer of the format a mask does not have (and of an absent mask or value field) is u's, in bounds for
                // either access: the fp32 read is then the load of u itself, the byte read hits the same lines
                if constexpr (MASK) {
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        w.mf[k][jb][n] = ld_at<float>(mfp[k], o);
                        w.mb[k][jb][n] = ld_at<uint8_t>(mbp[k], o);
                    }
                }
                if constexpr (BCF) {
#pragma unroll
                    for (int k = 0; k < 2; ++k) w.bf[k][jb][n] = ld_at<float>(bcfb[k], o);
                }
            }
    };
    // landed plane -> its stage: the two Dirichlet substitutions of u in order (condition 2 wins where both hold); the cotangent of a
    // Dirichlet node is zero, as the forward zeroes those rows
    auto plane_consume = [&](const Raw& w, Plane& S) {
        float v[2][2], l[2][2];
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                float t = w.u[jb][n];
                bool fixed = false;
                if constexpr (MASK) {
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const bool fx = p.mask_kind[k] == 2 ? (w.mf[k][jb][n] > 0.5f) : (p.mask_kind[k] == 1 ? (w.mb[k][jb][n] != 0) : false);
                        float bv = p.bcv[k];
                        if constexpr (BCF) bv = p.bcf[k] ? w.bf[k][jb][n] : bv;
                        t = fx ? bv : t;
                        fixed = fixed || fx;
                    }
                }
                v[jb][n] = t;
                if constexpr (VJP) l[jb][n] = fixed ? 0.f : w.l[jb][n] * lscale;
                if (jb == 0 && n == 0) S.keep = fixed ? 0.f : 1.f;
            }
        ek3_stage<NGP>(p, v[0][0], v[0][1], v[1][0], v[1][1], S.VU, S.VX, S.VY);
        if constexpr (VJP) ek3_stage<NGP>(p, l[0][0], l[0][1], l[1][0], l[1][1], S.LU, S.LX, S.LY);
        if constexpr (FN) ek3_stage_value<NGP>(p, w.f[0][0], w.f[0][1], w.f[1][0], w.f[1][1], S.VF);
        __builtin_amdgcn_sched_barrier(0);
    };

    // the upper-plane half of the last layer's transposed sums: value, x- and y-derivative coefficients at the in-plane Gauss points
    float cU[NGP][NGP], cX[NGP], cY[NGP];
#pragma unroll
    for (int j = 0; j < NGP; ++j) {
        cX[j] = cY[j] = 0.f;
#pragma unroll
        for (int i = 0; i < NGP; ++i) cU[j][i] = 0.f;
    }

    double sq_acc = 0.0;
    int par = 0;
    float pend_v = 0.f;                      // the last emitted plane's value, stored by flush_store() after the next request
    unsigned pend_off = 0u;
    bool pend_st = false;
    auto flush_store = [&]() {
        if (pend_st) st_at<float>(ob, pend_off, pend_v);
        pend_st = false;
    };
    const unsigned out_off = (unsigned)ey * (unsigned)p.nx + (unsigned)x0;

    // Node plane z is complete: the in-plane transpose of (cU, cX, cY) gives the element's contributions to its 2 x 2 nodes; those of
    // the nodes shared with the right, up and up-right threads go through LDS, the owner adds them in a fixed order
    auto emit_plane = [&](float keep, int z, bool owned_plane) {
        float r0[NGP], r1[NGP];               // per y-point: x-transposed onto node columns x0 and x0 + 1
#pragma unroll
        for (int j = 0; j < NGP; ++j) {
            float s = 0.f, t = 0.f;
#pragma unroll
            for (int i = 0; i < NGP; ++i) { s += cU[j][i]; t = fmaf(p.b1[i], cU[j][i], t); }
            const float xg = p.gx * cX[j];
            r1[j] = t + xg;
            r0[j] = (s - t) - xg;
        }
        float ys = 0.f, yt = 0.f;
#pragma unroll
        for (int i = 0; i < NGP; ++i) { const float yg = p.gy * cY[i]; ys += yg; yt = fmaf(p.b1[i], yg, yt); }
        float s0 = 0.f, t0 = 0.f, s1 = 0.f, t1 = 0.f;
#pragma unroll
        for (int j = 0; j < NGP; ++j) {
            s0 += r0[j]; t0 = fmaf(p.b1[j], r0[j], t0);
            s1 += r1[j]; t1 = fmaf(p.b1[j], r1[j], t1);
        }
        const float y0 = ys - yt, y1 = yt;
        const float o00 = elem_ok ? (s0 - t0) - y0 : 0.f, o01 = elem_ok ? (s1 - t1) - y1 : 0.f;
        const float o10 = elem_ok ? t0 + y0 : 0.f, o11 = elem_ok ? t1 + y1 : 0.f;
        xch[par][0][tid] = o01;
        xch[par][1][tid] = o10;
        xch[par][2][tid] = o11;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // LDS-only barrier (loads stay in flight)
        float t = o00;
        if (ty > 0) t += xch[par][1][tid - TX];
        if (tx > 0) t += xch[par][0][tid - 1];
        if (tx > 0 && ty > 0) t += xch[par][2][tid - TX - 1];
        t = keep > 0.f ? t : 0.f;               // nothing reaches a Dirichlet node (forward: the rows of R are zeroed; VJP: no gradient)
        const bool st = owned_plane && owner;
        sq_acc += st ? (double)(t * t) : 0.0;
        pend_v = t;
        pend_off = (unsigned)z * npl + out_off;
        pend_st = st && ob != nullptr;
        par ^= 1;
    };

    auto layer = [&](int ez, const Plane& L, const Plane& U) {
        float uU[NGP][NGP], uX[NGP], uY[NGP];
#pragma unroll
        for (int j = 0; j < NGP; ++j) {
            uX[j] = uY[j] = 0.f;
#pragma unroll
            for (int i = 0; i < NGP; ++i) uU[j][i] = 0.f;
        }
        const unsigned eo = (unsigned)ez * epl + eoff;
        // the z-points one after the other, as a loop: unrolled, the 3- and 4-point rules keep several z-points' factors alive and spill
#pragma nounroll
        for (int k = 0; k < NGP; ++k) {
            const float bk = p.b1[k];
            float fgk[FK == 2 ? NGP : 1][FK == 2 ? NGP : 1];
            if constexpr (FK == 2) {
#pragma unroll
                for (int j = 0; j < NGP; ++j)
#pragma unroll
                    for (int i = 0; i < NGP; ++i) fgk[j][i] = ld_at<float>(fgb, eo + (unsigned)((k * NGP + j) * NGP + i) * eps);
            }
            float ux[NGP], uy[NGP], lx[VJP ? NGP : 1], ly[VJP ? NGP : 1];
#pragma unroll
            for (int j = 0; j < NGP; ++j) {
                ux[j] = fmaf(bk, U.VX[j] - L.VX[j], L.VX[j]);
                uy[j] = fmaf(bk, U.VY[j] - L.VY[j], L.VY[j]);
                if constexpr (VJP) {
                    lx[j] = fmaf(bk, U.LX[j] - L.LX[j], L.LX[j]);
                    ly[j] = fmaf(bk, U.LY[j] - L.LY[j], L.LY[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < NGP; ++j)
#pragma unroll
                for (int i = 0; i < NGP; ++i) {
                    const float dU = U.VU[j][i] - L.VU[j][i];
                    const float v = fmaf(bk, dU, L.VU[j][i]), uz = p.gz * dU;
                    const float W = p.wji[j][i];
                    const float tv = p.tau * v;
                    float A, Bc, Cc, Dc;
                    if constexpr (VJP) {
                        const float dL = U.LU[j][i] - L.LU[j][i];
                        const float Lv = fmaf(bk, dL, L.LU[j][i]), lz = p.gz * dL;
                        const float s2L = p.sq2 * Lv;
                        A = p.tau * fmaf(lx[j], ux[j], fmaf(ly[i], uy[i], lz * uz));
                        Bc = fmaf(s2L, ux[j], tv * lx[j]);
                        Cc = fmaf(s2L, uy[i], tv * ly[i]);
                        Dc = fmaf(s2L, uz, tv * lz);
                    } else {
                        float f = p.fconst;
                        if constexpr (FK == 1) f = fmaf(bk, U.VF[j][i] - L.VF[j][i], L.VF[j][i]);
                        if constexpr (FK == 2) f = fgk[j][i];
                        A = fmaf(p.sq, fmaf(ux[j], ux[j], fmaf(uy[i], uy[i], uz * uz)), -f);
                        Bc = tv * ux[j];
                        Cc = tv * uy[i];
                        Dc = tv * uz;
                    }
                    const float cn = W * A, cx = W * Bc, cy = W * Cc, cz = W * Dc;
                    cU[j][i] = fmaf(-p.wgz[k], cz, fmaf(p.wb0[k], cn, cU[j][i]));
                    uU[j][i] = fmaf(p.wgz[k], cz, fmaf(p.wb1[k], cn, uU[j][i]));
                    cX[j] = fmaf(p.wb0[k], cx, cX[j]);
                    uX[j] = fmaf(p.wb1[k], cx, uX[j]);
                    cY[i] = fmaf(p.wb0[k], cy, cY[i]);
                    uY[i] = fmaf(p.wb1[k], cy, uY[i]);
                    // keep the Gauss points apart: left alone, the scheduler interleaves all of a layer's points and keeps every
                    // factor of every point alive (hundreds of spilled VGPRs at the 3- and 4-point rules)
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
        emit_plane(L.keep, ez, ez >= ez_own);
#pragma unroll
        for (int j = 0; j < NGP; ++j) {
            cX[j] = uX[j]; cY[j] = uY[j];
#pragma unroll
            for (int i = 0; i < NGP; ++i) cU[j][i] = uU[j][i];
        }
    };

    Plane SA, SB;
    {
        Raw W;
        plane_issue(ez_begin, W);
        plane_consume(W, SA);
        if constexpr (PF) plane_issue(ez_begin + 1, W);
        // two layers per trip with the roles of the two plane states swapped: no state copy at the end of a layer (planes beyond the
        // mesh re-read the last one, unused)
        int ez = ez_begin;
#pragma nounroll
        for (; ez + 1 < ez_end; ez += 2) {
            if constexpr (!PF) plane_issue(ez + 1, W);
            plane_consume(W, SB);
            if constexpr (PF) plane_issue(ez + 2, W);
            flush_store();
            layer(ez, SA, SB);
            if constexpr (!PF) plane_issue(ez + 2, W);
            plane_consume(W, SA);
            if constexpr (PF) plane_issue(ez + 3, W);
            flush_store();
            layer(ez + 1, SB, SA);
        }
        if (ez < ez_end) {
            if constexpr (!PF) plane_issue(ez + 1, W);
            plane_consume(W, SB);
            flush_store();
            layer(ez, SA, SB);
            SA = SB;
        }
        flush_store();
    }
    if (ez_end == p.nelz) {       // the last strip owns the top node plane: only the layer below contributes
        emit_plane(SA.keep, p.nz - 1, true);
        flush_store();
    }

    if (p.want_sums) {
        const int nthreads = TX * TY;
        double* parts[1] = {p.part};
        double mine[1] = {block_sum(sq_acc, red, tid, nthreads)}, tot[1];
        if (last_arriver_sums<1, 8, false, true>(parts, p.counter, mine, tid, nthreads, &last_flag, tot)) {
            const double e = block_sum(tot[0], red, tid, nthreads);
            if (tid == 0) {
                if (p.sumsq) p.sumsq[0] = e;
                if (p.norm) p.norm[0] = (float)sqrt(e);
                arrival_reset(p.counter);
                p.counter[DN_WS_TICKET_WORD] = 0u;
            }
        }
    }
}

// The forms of one rule: FK from the forcing pointers, MASK / BCF from the conditions, the VJP (FK == 0 only)
template <int NGP, int FK>
static void ek3_launch_mask(const Ek3Params& pp, dim3 grid, dim3 block, hipStream_t s) {
    const bool mask = pp.mask[0] || pp.mask[1], bcf = pp.bcf[0] || pp.bcf[1];
    if constexpr (FK == 0) {
        if (pp.vjp) {
            if (mask && bcf) hipLaunchKernelGGL((eikonal3d_kernel<NGP, true, true, 0, true>), grid, block, 0, s, pp);
            else if (mask) hipLaunchKernelGGL((eikonal3d_kernel<NGP, true, false, 0, true>), grid, block, 0, s, pp);
            else hipLaunchKernelGGL((eikonal3d_kernel<NGP, false, false, 0, true>), grid, block, 0, s, pp);
            return;
        }
    }
    if (mask && bcf) hipLaunchKernelGGL((eikonal3d_kernel<NGP, true, true, FK, false>), grid, block, 0, s, pp);
    else if (mask) hipLaunchKernelGGL((eikonal3d_kernel<NGP, true, false, FK, false>), grid, block, 0, s, pp);
    else hipLaunchKernelGGL((eikonal3d_kernel<NGP, false, false, FK, false>), grid, block, 0, s, pp);
}

template <int NGP>
void ek3_launch_forms(const Ek3Params& pp, dim3 grid, dim3 block, hipStream_t s) {
    if (pp.fgp) ek3_launch_mask<NGP, 2>(pp, grid, block, s);
    else if (pp.f) ek3_launch_mask<NGP, 1>(pp, grid, block, s);
    else ek3_launch_mask<NGP, 0>(pp, grid, block, s);
}

#ifndef EK3_NGP      // eikonal3d.hip itself compiles the 2-point rule; eikonal3d_g3.hip and eikonal3d_g4.hip the larger ones
extern template void ek3_launch_forms<3>(const Ek3Params&, dim3, dim3, hipStream_t);
extern template void ek3_launch_forms<4>(const Ek3Params&, dim3, dim3, hipStream_t);
#else
template void ek3_launch_forms<EK3_NGP>(const Ek3Params&, dim3, dim3, hipStream_t);
#endif

}  // namespace dn

#ifndef EK3_NGP
using namespace dn;

namespace {

struct Ek3Geom { int TX, TY, chunks, tiles, strips, R; };

inline int ek3_ceil_div(int a, int b) { return (a + b - 1) / b; }
// tiles of T threads that overlap by one thread cover n node columns (or rows)
inline int ek3_tiles(int n, int T) { return n <= T ? 1 : ek3_ceil_div(n - 1, T - 1); }

constexpr int EK3_MIN_PLANES = 4;          // shortest strip the library chooses (element planes): a strip recomputes one layer

// Tiles 16 threads wide; their height the multiple of 4 rows (whole waves) that wastes the fewest thread rows; the strip height
// halves from 32 planes until the launch has 1024 workgroups (4 per CU) or a strip has EK3_MIN_PLANES.  "PLAN3D" ("TX,TY,E,R", E
// ignored: one element per thread) overrides all three, as for dn_poisson_apply; the results do not depend on the plan.
Ek3Geom ek3_plan(const dn_mesh* m) {
    Ek3Geom g;
    const int nelz = m->nz - 1;
    g.TX = 16; g.TY = 16;
    double best = -1.0;
    for (int TY = 4; TY <= 16; TY += 4) {
        const double util = (double)m->ny / ((double)ek3_tiles(m->ny, TY) * TY) + 0.002 * TY;
        if (util > best) { best = util; g.TY = TY; }
    }
    int R = 32;
    const long long per_strip = (long long)ek3_tiles(m->nx, g.TX) * ek3_tiles(m->ny, g.TY) * m->batch;
    while (R > EK3_MIN_PLANES && per_strip * ek3_ceil_div(nelz, R) < 1024) R /= 2;
    const char* e = config(CFG_PLAN3D);
    int TX, TY, E, RR;
    if (e && sscanf(e, "%d,%d,%d,%d", &TX, &TY, &E, &RR) == 4 && TX >= 2 && TY >= 2 && TX * TY <= 256 && (TX * TY) % 64 == 0 && RR >= 1) {
        g.TX = TX; g.TY = TY; R = RR;
    }
    g.R = std::max(1, std::min(R, nelz));
    g.chunks = ek3_tiles(m->nx, g.TX);
    g.tiles = ek3_tiles(m->ny, g.TY);
    g.strips = ek3_ceil_div(nelz, g.R);
    return g;
}

int ek3_validate(const dn_mesh* m) {
    if (!m || m->nsd != 3) return DN_E_BADARG;
    if (m->degree != 1 || m->ngp < 2 || m->ngp > 4) return DN_E_UNSUPPORTED;
    if (m->batch < 1 || m->batch > 65535 || m->nx < 2 || m->ny < 2 || m->nz < 2) return DN_E_BADARG;
    if ((int64_t)m->nx * m->ny * m->nz >= (1ll << 30)) return DN_E_UNSUPPORTED;          // 32-bit in-sample byte offsets
    return 0;
}

int64_t ek3_workspace_bytes(const dn_mesh* m, const Ek3Geom& g) {
    return DN_WS_HEADER + (int64_t)sizeof(double) * g.chunks * g.tiles * g.strips * m->batch;
}

}  // namespace

extern "C" int64_t dn_eikonal3d_workspace_bytes(const dn_mesh* m) {
    if (ek3_validate(m) != 0) return DN_E_BADARG;
    return ek3_workspace_bytes(m, ek3_plan(m));
}

extern "C" int dn_eikonal3d_apply(const dn_mesh* m, const dn_eikonal_args* a, void* stream) {
    int rc = ek3_validate(m);
    if (rc) return rc;
    if (!a || !a->u) return DN_E_BADARG;
    if (!a->out && !a->sumsq && !a->norm) return DN_E_BADARG;
    if ((a->in_den && !a->in_num) || (a->vjp & ~1)) return DN_E_BADARG;
    const bool vjp = a->vjp != 0;
    if (vjp && !a->cot) return DN_E_BADARG;                                  // a VJP without its cotangent
    if (!vjp && a->in_num) return DN_E_BADARG;                               // the scaling applies to the cotangent only
    if ((rc = elem_check_conditions(a)) != 0) return rc;
    const int64_t nel = (int64_t)(m->nx - 1) * (m->ny - 1) * (m->nz - 1);
    if (a->f_gp && !vjp && nel * m->ngp * m->ngp * m->ngp >= (1ll << 30)) return DN_E_UNSUPPORTED;
    const Ek3Geom g = ek3_plan(m);
    const bool sums = a->sumsq || a->norm;
    if (sums && (!a->workspace || a->workspace_bytes < ek3_workspace_bytes(m, g))) return DN_E_WORKSPACE;
    const long long nwg = (long long)g.chunks * g.tiles * g.strips * m->batch;
    if (nwg >= (1ll << 31)) return DN_E_UNSUPPORTED;

    Ek3Params pp;
    for (int i = 0; i < 4; ++i) {
        pp.b1[i] = i < m->ngp ? m->basis[i][1] : 0.f;
        pp.wb0[i] = i < m->ngp ? m->gpw[i] * m->basis[i][0] : 0.f;
        pp.wb1[i] = i < m->ngp ? m->gpw[i] * m->basis[i][1] : 0.f;
        pp.wgz[i] = i < m->ngp ? (float)((double)m->gpw[i] * m->dbasis[0][1] * m->scale[2]) : 0.f;
        for (int j = 0; j < 4; ++j) pp.wji[i][j] = (i < m->ngp && j < m->ngp) ? m->gpw[i] * (m->gpw[j] * a->wscale) : 0.f;
    }
    pp.gx = (float)((double)m->dbasis[0][1] * m->scale[0]);
    pp.gy = (float)((double)m->dbasis[0][1] * m->scale[1]);
    pp.gz = (float)((double)m->dbasis[0][1] * m->scale[2]);
    pp.tau = a->tau; pp.sq = a->sq; pp.sq2 = 2.f * a->sq;
    pp.fconst = (a->f || a->f_gp) ? 0.f : a->f_value;
    pp.u = a->u;
    pp.cot = vjp ? a->cot : nullptr;
    pp.in_num = a->in_num; pp.in_den = a->in_den;
    elem_fill_conditions(pp, a);
    if (vjp) pp.f = pp.fgp = nullptr;                                        // the VJP does not read the forcing
    pp.out = a->out; pp.sumsq = a->sumsq; pp.norm = a->norm;
    pp.nx = m->nx; pp.ny = m->ny; pp.nz = m->nz;
    pp.nelx = m->nx - 1; pp.nely = m->ny - 1; pp.nelz = m->nz - 1;
    pp.rows_per_strip = g.R;
    pp.want_sums = sums ? 1 : 0;
    pp.chunks_x = g.chunks; pp.tiles_y = g.tiles; pp.strips_z = g.strips;
    pp.vjp = a->vjp;

    const dim3 grid((unsigned)nwg), block(g.TX, g.TY);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (m->ngp) {
        case 2: ek3_launch_forms<2>(pp, grid, block, s); break;
        case 3: ek3_launch_forms<3>(pp, grid, block, s); break;
        default: ek3_launch_forms<4>(pp, grid, block, s); break;
    }
    DN_LAUNCH_CHECK();
    return 0;
}
#endif
