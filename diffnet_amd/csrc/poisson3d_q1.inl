// 3-D Q1 fused Poisson kernel, fully sum-factorised marching form.  Included by
// poisson3d_q1_g{2,3,4}.hip with DN_NGP defined.
//
// grid = chunks_x * tiles_y * strips_z * B workgroups (strip3d_decode), block = (TX, TY).  Thread (tx, ty) owns one element of element
// row ey (poisson3d_q1n2_kernel: two) and marches over element planes.  Carried per element: the in-plane stage of the lower node plane
// (VU/VX/VY/VN/VF at the in-plane Gauss points) and the cotangents of that plane's stage values from the layer
// below.  Per layer: load the two node rows of the new plane, x- and y-stage them, the O(NGP^2) layer arithmetic
// (q1_layer_3d_w), then ONE in-plane transpose (y then x) per finished plane; contributions to nodes shared with the
// neighbouring threads (right, up, up-right) go through a double-buffered LDS slot, one LDS-only barrier per layer.
#include <cstdlib>

#include "poisson3d_q1_common.h"

namespace dn {

// pure 1-D weight of Gauss point g (1 at compile time for the unit-weight rule)
#define T_W(T, g, UW) ((UW) ? 1.f : (T).w[g])

// =============================================================================================================
// Second-generation kernel (the round-1 kernel it replaced -- poisson3d_q1m_kernel, ~1/3 more VALU instructions per element -- is no longer
// in the tree; its numbers stay in profiles/r1_*): same mapping, hand-over and reductions.
//   * coefficient planes are staged WEIGHTED (w_j w_i nu, w_j w_i f) together with their in-plane sums A[j], B[i], once per
//     plane; the layer arithmetic (q1_layer_3d_w) works on raw differences and applies 1/h^2, alpha and the user scale
//     once per element; carried cotangents are folded into the layer's own fused multiply-adds;
//   * UW (exact 2-point rule, all weights 1): every weight multiplication vanishes at compile time;
//   * every global access is SGPR base + 32-bit byte offset (ld_at / st_at): no 64-bit VALU address arithmetic.
// =============================================================================================================
template <int NGP>
struct PlaneW {
    float VU[NGP][NGP], VX[NGP], VY[NGP];
    float VN[NGP][NGP];                               // weighted nu at the in-plane Gauss points
    float VF[NGP][NGP];                               // weighted f
    float keep;                                       // 0 where the thread's own node is a Dirichlet node
};

// in-plane stage of u for one element: nodal values r0[e], r0[e+1] (row ey) and r1[e], r1[e+1] (row ey + 1).
// V = float, or v2f: two elements at once in the halves of packed-fp32 registers (v_pk_fma_f32 ...)
template <int NGP, typename V = float>
__device__ __forceinline__ void stage_u3(const ElemTab& T, V a0, V a1, V b0, V b1, V (&VU)[NGP][NGP], V (&VX)[NGP], V (&VY)[NGP]) {
    const V dx0 = a1 - a0, dx1 = b1 - b0, ddx = dx1 - dx0;
#pragma unroll
    for (int j = 0; j < NGP; ++j) VX[j] = vfma(T.b[j][1], ddx, dx0);
#pragma unroll
    for (int i = 0; i < NGP; ++i) {
        const V t0 = vfma(T.b[i][1], dx0, a0);
        VY[i] = vfma(T.b[i][1], dx1, b0) - t0;
#pragma unroll
        for (int j = 0; j < NGP; ++j) VU[j][i] = vfma(T.b[j][1], VY[i], t0);
    }
}

// weighted in-plane stage of a coefficient field: V[j][i] = w_j w_i * c(gp j, i)
template <int NGP, bool UW, typename V = float>
__device__ __forceinline__ void stage_w3(const ElemTab& T, V a0, V a1, V b0, V b1, V (&W)[NGP][NGP]) {
    const V dx0 = a1 - a0, dx1 = b1 - b0;
#pragma unroll
    for (int i = 0; i < NGP; ++i) {
        V t0, t1;
        if constexpr (UW) {
            t0 = vfma(T.b[i][1], dx0, a0);
            t1 = vfma(T.b[i][1], dx1, b0);
        } else {
            t0 = vfma(T.wb[i], dx0, T.w[i] * a0);
            t1 = vfma(T.wb[i], dx1, T.w[i] * b0);
        }
        const V dy = t1 - t0;
#pragma unroll
        for (int j = 0; j < NGP; ++j) W[j][i] = UW ? vfma(T.b[j][1], dy, t0) : vfma(T.wb[j], dy, T.w[j] * t0);
    }
}

// T16: one element per thread in tiles exactly 16 threads wide.  A thread row is then a DPP row, so the hand-over to the right
// neighbour is a `row_shr:1` move (zero fill at the tile's left edge) instead of an LDS slot, the up-right hand-over folds into
// the up slot, and a thread's two nodes per row come from ONE (4-byte aligned) dwordx2 / ushort load.
struct __attribute__((packed, aligned(4))) F2U { float a, b; };
struct __attribute__((packed, aligned(1))) B2U { uint8_t a, b; };

// One element per thread, tiles of any shape (generic) or exactly 16 threads wide (T16).
// Waves per SIMD asked of the compiler: 5 = the 16-wide form with the next plane's loads in flight (<= 96 VGPRs), 6 = the generic form at
// 2 x 2 x 2 points (<= 80 VGPRs), 4 = either with value fields, mixed masks or Gauss-point forcing (<= 128 VGPRs); 3 / 4 and 2 at 3 and 4 points
template <int NGP, int FL, bool UW, bool T16>
__global__ void __launch_bounds__(256, NGP == 4 ? 2 : (NGP == 3 ? (T16 ? 3 : 4) : ((FL & (FL3_BC | FL3_FGP)) ? 4 : (T16 ? 5 : 6)))) poisson3d_q1w_kernel(const PoissonParams p, const int chunks_x, const int tiles_y,
                                                                            const int strips_z) {
    constexpr int G = NGP * NGP * NGP;
    constexpr bool HAS_NU = (FL & FL3_NU) != 0, HAS_F = (FL & FL3_F) != 0, FGP = (FL & FL3_FGP) != 0;
    constexpr bool BC_U8C = (FL & FL3_BC_U8C) != 0, BC_ANY = (FL & (FL3_BC | FL3_BC_U8C)) != 0;
    const int TX = blockDim.x, TY = blockDim.y;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int tid = ty * TX + tx;
    const Strip3D wg = strip3d_decode(xcd_remap(blockIdx.x, gridDim.x), chunks_x, tiles_y, strips_z, p.strip_sel, p.nstrips, p.rows_per_strip, p.nelz);
    const int chunk = wg.chunk, tile = wg.tile, b = wg.b, ez_own = wg.ez_own, ez_begin = wg.ez_begin, ez_end = wg.ez_end;
    const int x0 = chunk * (TX - 1) + tx;
    const int ey = tile * (TY - 1) + ty;
    const bool owner = !(chunk > 0 && tx == 0) && !(tile > 0 && ty == 0);
    const unsigned npl = (unsigned)(p.nx * p.ny);
    const int64_t nps = (int64_t)npl * p.nz;
    const unsigned epl = (unsigned)(p.nelx * p.nely);
    const unsigned eps = epl * (unsigned)p.nelz;
    const SampleBases sb = sample_bases(p, b, nps);
    const float* fgp = FGP ? p.fgp + (p.f_batched ? (int64_t)b * eps * G : 0) : nullptr;
    const bool noderow_ok = ey < p.ny;
    // Elements beyond the mesh (ragged right / upper edge of the last chunk / tile) are computed like any other on clamped,
    // finite node values and their results multiplied by 0: no per-element branches, no exec-masked regions in the loop.
    const float okf = (ey < p.nely && x0 < p.nelx) ? 1.f : 0.f;

    __shared__ float xch[2][T16 ? 1 : 3][256];      // hand-over slots: right, up, up-right (T16: up)
    __shared__ double red[2 * (256 / 64)];      // block_sum2: two sums per wave
    __shared__ int last_flag;

    PlaneW<NGP> SA, SB;
    float cU[NGP][NGP], cX[NGP], cY[NGP];
    SA.keep = SB.keep = 1.f;
#pragma unroll
    for (int j = 0; j < NGP; ++j) {
        cX[j] = cY[j] = 0.f;
#pragma unroll
        for (int i = 0; i < NGP; ++i) {
            cU[j][i] = 0.f;
            SA.VN[j][i] = SB.VN[j][i] = T_W(p.T, j, UW) * T_W(p.T, i, UW);    // nu absent: the constant field 1
            SA.VF[j][i] = SB.VF[j][i] = 0.f;
        }
    }

    // byte offsets of this thread's two node rows inside a plane; the plane offset is added per plane (one VALU add each)
    const int y0c = min(ey, p.ny - 1), y1c = min(ey + 1, p.ny - 1);
    const unsigned row0 = (unsigned)y0c * (unsigned)p.nx, row1 = (unsigned)y1c * (unsigned)p.nx;
    const unsigned x0c = (unsigned)min(x0, p.nx - 2);         // T16: in-bounds start of the thread's node pair
    const bool pair_shifted = x0 == p.nx - 1;                  // T16: owner of the last node column (no element of its own)

    // Raw node values of one plane (this thread's two rows), as loaded: `plane_issue` only issues the loads, `plane_consume`
    // applies the Dirichlet conditions and stages.  PF (T16 form): the loads of plane k + 2 are issued BEFORE the arithmetic of
    // layer k and consumed after it, so a wave does not sit on its memory latency once per layer (rocprofv3: 64 % of the wave
    // cycles were s_waitcnt / barrier waits without it); 14 more live VGPRs at one element per thread.
    // uint8 masks with constant values: both mask slots are always loaded (mask_images)
    const MaskImages mi = mask_images(sb.mask[0], sb.mask[1]);
    struct RawPlane {
        float ru[2][2], rn[2][2], rf[2][2];      // [node row][node column]
        BcRaw<1> braw[2];
        uint8_t m8[2][2][2];
    };
    auto plane_issue = [&](int zreq, RawPlane& W) {
        const unsigned zoff = (unsigned)min(zreq, p.nz - 1) * npl;
        const unsigned rowoff[2] = {zoff + row0, zoff + row1};
        float (&ru)[2][2] = W.ru;
        float (&rn)[2][2] = W.rn;
        float (&rf)[2][2] = W.rf;
        BcRaw<1> (&braw)[2] = W.braw;
        uint8_t (&m8)[2][2][2] = W.m8;
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            if constexpr (T16) {
                // both nodes of the row in one load; threads right of the mesh read the last valid pair (their element is masked)
                const unsigned o2 = rowoff[jb] + x0c;
                // one 4-byte-aligned dwordx2 / ushort per node pair; two aligned dword loads instead measured 165 -> 249 us at 256^3: the second
                // load hits lines still in flight (profiles/r2_3d_bottleneck.md)
                const F2U a = ld_at<F2U>(sb.u, o2);
                ru[jb][0] = a.a; ru[jb][1] = a.b;
                if constexpr (HAS_NU) { const F2U t = ld_at<F2U>(sb.nu, o2); rn[jb][0] = t.a; rn[jb][1] = t.b; }
                if constexpr (HAS_F) { const F2U t = ld_at<F2U>(sb.f, o2); rf[jb][0] = t.a; rf[jb][1] = t.b; }
                if constexpr (BC_U8C) {
                    // unconditional loads, no load inside a uniform branch (an absent mask reads the other one and is ignored: mask_images)
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const B2U t = ld_at<B2U>(mi.m8[k], o2);
                        m8[jb][k][0] = t.a; m8[jb][k][1] = t.b;
                    }
                } else if constexpr (BC_ANY) {
                    bc_issue<1, false>(p, sb, rowoff[jb], (int)x0c, braw[jb]);
                }
            } else {
                load_seg<1, false>(sb.u, rowoff[jb], x0, p.nx, ru[jb]);
                if constexpr (HAS_NU) load_seg<1, false>(sb.nu, rowoff[jb], x0, p.nx, rn[jb]);
                if constexpr (HAS_F) load_seg<1, false>(sb.f, rowoff[jb], x0, p.nx, rf[jb]);
                if constexpr (BC_U8C) {
#pragma unroll
                    for (int k = 0; k < 2; ++k) load_seg<1, false>(mi.m8[k], rowoff[jb], x0, p.nx, m8[jb][k]);
                } else if constexpr (BC_ANY) {
                    bc_issue<1, false>(p, sb, rowoff[jb], x0, braw[jb]);
                }
            }
        }
    };
    auto plane_consume = [&](RawPlane& W, PlaneW<NGP>& S) {
        float (&ru)[2][2] = W.ru;
        float (&rn)[2][2] = W.rn;
        float (&rf)[2][2] = W.rf;
        BcRaw<1> (&braw)[2] = W.braw;
        uint8_t (&m8)[2][2][2] = W.m8;
        float kall[2] = {1.f, 1.f};           // 0 on Dirichlet nodes of row ey (both loaded nodes)
        if constexpr (BC_U8C) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float val = p.bc[k].value;
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const bool set = mi.has[k] && m8[jb][k][n] != 0;
                        ru[jb][n] = set ? val : ru[jb][n];
                        if (jb == 0) kall[n] = set ? 0.f : kall[n];
                    }
            }
        } else if constexpr (BC_ANY) {
            float k1[2];
            bc_apply_all<1>(p, sb, braw[0], ru[0], kall);
            bc_apply_all<1>(p, sb, braw[1], ru[1], k1);
        }
        // T16: the thread of the last node column loads the pair (nx-2, nx-1); the node it owns is the second one
        S.keep = (T16 && pair_shifted) ? kall[1] : kall[0];
        // (A loop of one trip, on purpose: with the three calls written straight into the lambda the two 4-point generic kernels with nu and
        // Gauss-point forcing spill 480 / 484 bytes per lane instead of 324 / 328 under ROCm 7.2's compiler (AMD clang 22.0.0git, roc-7.2.0) --
        // profiles/poisson3d_refactor.txt.  Try the plain form again with a newer compiler.)
#pragma unroll
        for (int e = 0; e < 1; ++e) {
            stage_u3<NGP>(p.T, ru[0][e], ru[0][e + 1], ru[1][e], ru[1][e + 1], S.VU, S.VX, S.VY);
            if constexpr (HAS_NU) stage_w3<NGP, UW>(p.T, rn[0][e], rn[0][e + 1], rn[1][e], rn[1][e + 1], S.VN);
            if constexpr (HAS_F) stage_w3<NGP, UW>(p.T, rf[0][e], rf[0][e + 1], rf[1][e], rf[1][e + 1], S.VF);
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    auto plane_stage = [&](int zreq, PlaneW<NGP>& S) {
        RawPlane W;
        plane_issue(zreq, W);
        plane_consume(W, S);
    };

    float e1_acc = 0.f, e2_acc = 0.f, sq_acc = 0.f;
    int par = 0;

    const unsigned out_row = (unsigned)ey * (unsigned)p.nx;
    const int from_left = (int)(((unsigned)tid - 1u) & 63u) << 2;      // T16 hand-over: source lane of lane_from_left
    const float nfirst = tx > 0 ? 1.f : 0.f;
    float pend_v = 0.f;                       // T16: output of the last emitted plane, not yet stored
    unsigned pend_off = 0u;
    bool pend_st = false;
    auto flush_store = [&]() {
        if (pend_st) st_at<float>(sb.out, pend_off, pend_v);
        pend_st = false;
    };
    auto emit_plane = [&](const float (&o)[2][2], float keep, int z, bool owned_plane) {
        if constexpr (T16) {
            const float left = lane_from_left(o[0][1], from_left, nfirst);          // right-hand contribution of the thread to the left
            xch[par][0][tid] = o[1][0] + lane_from_left(o[1][1], from_left, nfirst);        // up slot with the up-right part of the left thread folded in
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            // the value is stored by flush_store(), AFTER the next plane has been consumed and the one after it requested: a
            // store issued here would be younger than those loads' consumer wait, which the compiler turns into vmcnt(0)
            float t = o[0][0] + left;
            if (ty > 0) t += xch[par][0][tid - 16];
            t *= keep;
            const bool st = owned_plane && owner && noderow_ok;
            sq_acc = st ? fmaf(t, t, sq_acc) : sq_acc;
            pend_v = t * p.out_scale;
            pend_off = (unsigned)z * npl + out_row + (unsigned)x0;
            pend_st = st && sb.out != nullptr && x0 < p.nx;
        } else {
            xch[par][0][tid] = o[0][1];
            xch[par][1][tid] = o[1][0];
            xch[par][2][tid] = o[1][1];
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (owned_plane && owner && noderow_ok) {
                float t = o[0][0];
                if (ty > 0) t += xch[par][1][tid - TX];
                if (tx > 0) t += xch[par][0][tid - 1];
                if (tx > 0 && ty > 0) t += xch[par][2][tid - TX - 1];
                t *= keep;
                sq_acc = fmaf(t, t, sq_acc);
                const float v[1] = {t * p.out_scale};
                if (sb.out) store_seg<1, false>(sb.out, (unsigned)z * npl + out_row, x0, p.nx, v);
            }
        }
        par ^= 1;
    };

    auto layer = [&](int ez, const PlaneW<NGP>& L, const PlaneW<NGP>& U) {
        const bool own_layer = ez >= ez_own;
        const float cnt = (own_layer && owner) ? 1.f : 0.f;
        float o[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, fg[G];
        if constexpr (FGP) {
            const unsigned eo = (unsigned)ez * epl + (unsigned)min(ey, p.nely - 1) * (unsigned)p.nelx + (unsigned)min(x0, p.nelx - 1);
#pragma unroll
            for (int gi = 0; gi < G; ++gi) fg[gi] = ld_at<float>(fgp, eo + (unsigned)gi * eps);
        }
        float tU[NGP][NGP], tX[NGP], tY[NGP], e1, e2;
        q1_layer_3d_w<NGP, FGP, HAS_F, UW>(p.T, L.VU, U.VU, L.VX, U.VX, L.VY, U.VY, L.VN, U.VN, L.VF, U.VF, fg, cU, cX, cY, tU, tX, tY, e1, e2);
        // pin the element's energy sums here: left alone, the compiler sinks their fused multiply-adds to the end of the layer
        // and keeps every Gauss-point factor alive until then (232 VGPRs instead of ~110)
        asm volatile("" : "+v"(e1), "+v"(e2));
        const float le1 = fmaf(okf, e1, 0.f), le2 = fmaf(okf, e2, 0.f);
        plane_transpose<NGP, float, true>(p.T.b, okf, tU, tX, tY, o);
        __builtin_amdgcn_sched_barrier(0);      // the element arithmetic stays ahead of the hand-over (the kernels were measured with this fence)
        e1_acc = fmaf(cnt, le1, e1_acc);
        e2_acc = fmaf(cnt, le2, e2_acc);
        emit_plane(o, L.keep, ez, own_layer);
    };

    plane_stage(ez_begin, SA);
    if constexpr (T16) {
        // software pipeline: plane k + 2 is in flight while layer k is computed (planes beyond the mesh re-read the last one)
        RawPlane W;
        plane_issue(ez_begin + 1, W);
        int ez = ez_begin;
#pragma nounroll
        for (; ez + 1 < ez_end; ez += 2) {
            plane_consume(W, SB);
            plane_issue(ez + 2, W);
            flush_store();
            layer(ez, SA, SB);
            plane_consume(W, SA);
            plane_issue(ez + 3, W);
            flush_store();
            layer(ez + 1, SB, SA);
        }
        if (ez < ez_end) {
            plane_consume(W, SB);
            flush_store();
            layer(ez, SA, SB);
            SA = SB;
        }
        flush_store();
    } else {
        // two layers per trip with the roles of the two plane states swapped: no state copy at the end of a layer
        int ez = ez_begin;
#pragma nounroll
        for (; ez + 1 < ez_end; ez += 2) {
            plane_stage(ez + 1, SB);
            layer(ez, SA, SB);
            plane_stage(ez + 2, SA);
            layer(ez + 1, SB, SA);
        }
        if (ez < ez_end) {
            plane_stage(ez + 1, SB);
            layer(ez, SA, SB);
            SA = SB;
        }
    }
    if (ez_end == p.nelz) {       // the last strip owns the top boundary plane: only the layer below contributes
        float o[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
        plane_transpose<NGP, float, true>(p.T.b, okf, cU, cX, cY, o);
        emit_plane(o, SA.keep, p.nz - 1, true);
        if constexpr (T16) flush_store();
    }

    if (p.want_sums) finish_sums(p, e1_acc, e2_acc, sq_acc, tid, TX * TY, red, &last_flag, (double)p.T.esc);
}

// =============================================================================================================
// Third form (default for nodal / absent forcing and no or uint8 constant-value conditions): EVERY NODE IS REQUESTED ONCE per
// workgroup and plane.  The T16 form above asks for every node four times (two rows x two columns of threads, misaligned
// dwordx2 / ushort pairs): 182 TA-cycles per wave and layer, which is what bounds it (profiles/r2_3d_bottleneck.md).  Here a thread
// loads only the node it owns -- aligned dword / byte loads, 4 rows x 16 lanes per wave-instruction --, applies the Dirichlet
// conditions to it once, and publishes {u', nu, f, keep} as one 16-byte record in an LDS tile of 17 x 17 nodes; the 33 halo nodes
// of the tile (column 16, row 16) are loaded 9 per wave by lanes 0..8 of the same unconditional instructions.  After the barrier
// the hand-over needs anyway, a thread reads the four records of its element with ds_read_b128.  One barrier per layer:
//     request plane k + 2  ->  gather + stage plane k + 1 from LDS  ->  layer k  ->  publish plane k + 2, hand-over  ->  barrier  ->  finish plane k
// =============================================================================================================
// 2 x 2 x 2 points: 5 waves per SIMD (<= 96 VGPRs).  The 3- and 4-point rules get 3 / 2 (<= 168 / 256 VGPRs): at 5 they spilled 100-500 bytes of
// scratch per thread
template <int NGP, int FL, bool UW>
__global__ void __launch_bounds__(256, NGP == 2 ? 5 : (NGP == 3 ? 3 : 2)) poisson3d_q1n_kernel(const PoissonParams p, const int chunks_x, const int tiles_y, const int strips_z) {
    constexpr bool HAS_NU = (FL & FL3_NU) != 0, HAS_F = (FL & FL3_F) != 0, BC_U8C = (FL & FL3_BC_U8C) != 0;
    constexpr int NMASK = !BC_U8C ? 0 : ((FL & FL3_BC_ONE) ? 1 : 2);
    constexpr bool MASK_F32 = (FL & FL3_BC_F32) != 0;
    // FL3_E1G: the stiffness part of the energy is not summed Gauss point by Gauss point but taken from the finished nodal values:
    // sum_a u_a out_a = alpha * sum W nu |grad u|^2 - beta * sum W f u  (u = sum_a u_a N_a), one FMA per node instead of 15 per element
    constexpr bool E1G = (FL & FL3_E1G) != 0;     // uint8 mask arrays read per node (compile-time: no load in a uniform branch)
    static_assert((FL & (FL3_FGP | FL3_BC)) == 0, "node-owner form: nodal forcing, uint8 constant-value conditions");
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int tid = ty * 16 + tx;
    const Strip3D wg = strip3d_decode(xcd_remap(blockIdx.x, gridDim.x), chunks_x, tiles_y, strips_z, p.strip_sel, p.nstrips, p.rows_per_strip, p.nelz);
    const int chunk = wg.chunk, tile = wg.tile, b = wg.b, ez_own = wg.ez_own, ez_begin = wg.ez_begin, ez_end = wg.ez_end;
    const int nx0 = chunk * 15, ny0 = tile * 15;               // first node of the tile
    const int x0 = nx0 + tx, ey = ny0 + ty;                    // the thread's node == lower-left node of its element
    const bool owner = !(chunk > 0 && tx == 0) && !(tile > 0 && ty == 0);
    const unsigned npl = (unsigned)(p.nx * p.ny);
    const int64_t nps = (int64_t)npl * p.nz;
    const SampleBases sb = sample_bases(p, b, nps);
    const bool noderow_ok = ey < p.ny;
    const float okf = (ey < p.nely && x0 < p.nelx) ? 1.f : 0.f;         // elements beyond the mesh: computed on clamped data, scaled by 0

    // (The 1-D tables the loop multiplies with in VECTOR registers instead of SGPR operands measured equal, 103 VGPRs: this kernel's waves do
    // not pair anyway, its layer period is the sum of its phases -- profiles/r2_prio3d.txt, profiles/r2_valu_sgpr.txt.)
    ElemTab TV = p.T;
    __shared__ float4 rec[2][17 * 17];            // [plane parity][node row * 17 + node column] = {u after Dirichlet, nu, f, keep}
    __shared__ float xch[2][256];
    __shared__ double red[2 * (256 / 64)];      // block_sum2: two sums per wave
    __shared__ int last_flag;

    // in-plane offsets (nodes, clamped into the mesh) of the node this thread owns and of the halo node it fetches
    const unsigned own_off = (unsigned)min(ey, p.ny - 1) * (unsigned)p.nx + (unsigned)min(x0, p.nx - 1);
    const int lane = tid & 63, wave = tid >> 6;
    // 33 halo nodes, 9 per wave; their u, nu and f come from ONE load instruction: lanes 0..8 fetch u, 9..17 nu, 18..26 f of the wave's nine nodes
    // through per-lane 64-bit addresses (round 3: a vector-memory instruction costs a wave ~64 cycles of issue whatever its active lanes); the
    // other lanes repeat lane 26.  Each lane writes its one component of the halo record.
    const int hgrp = min(lane / 9, 2), hsub = min(lane - 9 * hgrp, 8);
    const int hidx = min(wave * 9 + hsub, 32);
    const int hrow = hidx < 16 ? hidx : 16, hcol = hidx < 16 ? 16 : hidx - 16;
    const unsigned halo_off = (unsigned)min(ny0 + hrow, p.ny - 1) * (unsigned)p.nx + (unsigned)min(nx0 + hcol, p.nx - 1);
    const bool halo_lane = lane < 27 && wave * 9 + hsub < 33 && (hgrp == 0 || (hgrp == 1 ? HAS_NU : HAS_F));
    const int own_rec = ty * 17 + tx, halo_rec = hrow * 17 + hcol;
    const float* const halo_src = (hgrp == 1 && HAS_NU) ? sb.nu : ((hgrp == 2 && HAS_F) ? sb.f : sb.u);       // per lane

    const MaskImages mi = mask_images(sb.mask[0], sb.mask[1]);
    // with one condition, slot 0 of mi.m8 / bcval is the one that is present
    const float bcval[2] = {NMASK == 1 ? (mi.has[0] ? p.bc[0].value : p.bc[1].value) : p.bc[0].value, p.bc[1].value};
    struct RawNodes { float u, n, f, h; uint8_t m[2][2]; float mf[2][2]; };       // own node: u, n, f; halo node: h (u, nu or f by lane group); masks [0] own, [1] halo
    auto plane_request = [&](int zreq, RawNodes& W) {
        const unsigned zoff = (unsigned)min(zreq, p.nz - 1) * npl;
        const unsigned o[2] = {zoff + own_off, zoff + halo_off};
        W.u = ld_at<float>(sb.u, o[0]);
        if constexpr (HAS_NU) W.n = ld_at<float>(sb.nu, o[0]);
        if constexpr (HAS_F) W.f = ld_at<float>(sb.f, o[0]);
        W.h = halo_src[o[1]];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if constexpr (BC_U8C) {
#pragma unroll
                for (int k = 0; k < NMASK; ++k) {
                    if constexpr (MASK_F32) W.mf[h][k] = ld_at<float>(mi.m32[k], o[h]);
                    else W.m[h][k] = ld_at<uint8_t>(mi.m8[k], o[h]);
                }
            }
        }
    };
    auto plane_publish = [&](const RawNodes& W, int zpl) {
        float uu = W.u, keep = 1.f, hv = W.h;
        if constexpr (BC_U8C) {
#pragma unroll
            for (int k = 0; k < NMASK; ++k) {
                const bool set = (NMASK == 1 || mi.has[k]) && (MASK_F32 ? W.mf[0][k] > 0.5f : W.m[0][k] != 0);
                uu = set ? bcval[k] : uu;
                keep = set ? 0.f : keep;
                const bool seth = hgrp == 0 && (NMASK == 1 || mi.has[k]) && (MASK_F32 ? W.mf[1][k] > 0.5f : W.m[1][k] != 0);
                hv = seth ? bcval[k] : hv;
            }
        }
        rec[zpl & 1][own_rec] = make_float4(uu, HAS_NU ? W.n : 1.f, HAS_F ? W.f : 0.f, keep);
        // (the .w of a halo record is never read; absent nu / f keep the 1 / 0 the prologue put there)
        if (halo_lane) reinterpret_cast<float*>(&rec[zpl & 1][halo_rec])[hgrp] = hv;
    };
    float ut_acc = 0.f;                           // E1G: sum of u * out over the owned nodes
    struct PlaneN : PlaneW<NGP> { float uown; };      // uown: the own node's value after the Dirichlet conditions (E1G)
    auto plane_gather = [&](int zpl, PlaneN& S) {
        const float4* t = &rec[zpl & 1][own_rec];
        const float4 a0 = t[0], a1 = t[1], b0 = t[17], b1 = t[18];
        S.keep = a0.w;
        S.uown = a0.x;
        stage_u3<NGP>(TV, a0.x, a1.x, b0.x, b1.x, S.VU, S.VX, S.VY);
        if constexpr (HAS_NU) stage_w3<NGP, UW>(TV, a0.y, a1.y, b0.y, b1.y, S.VN);
        if constexpr (HAS_F) stage_w3<NGP, UW>(TV, a0.z, a1.z, b0.z, b1.z, S.VF);
        __builtin_amdgcn_sched_barrier(0);
    };

    PlaneN SA, SB;
    float cU[NGP][NGP], cX[NGP], cY[NGP];
    SA.keep = SB.keep = 1.f;
    SA.uown = SB.uown = 0.f;
#pragma unroll
    for (int j = 0; j < NGP; ++j) {
        cX[j] = cY[j] = 0.f;
#pragma unroll
        for (int i = 0; i < NGP; ++i) {
            cU[j][i] = 0.f;
            SA.VN[j][i] = SB.VN[j][i] = T_W(TV, j, UW) * T_W(TV, i, UW);    // nu absent: the constant field 1
            SA.VF[j][i] = SB.VF[j][i] = 0.f;
        }
    }

    float e1_acc = 0.f, e2_acc = 0.f, sq_acc = 0.f;
    int par = 0;

    const unsigned out_row = (unsigned)ey * (unsigned)p.nx;
    const int from_left = (int)(((unsigned)tid - 1u) & 63u) << 2;
    const float nfirst = tx > 0 ? 1.f : 0.f;
    float pend_v = 0.f;
    unsigned pend_off = 0u;
    bool pend_st = false;
    auto flush_store = [&]() {
        if (pend_st) st_at<float>(sb.out, pend_off, pend_v);
        pend_st = false;
    };
    // hand the finished contributions over, (optionally) publish the plane requested at the top of the layer, ONE barrier, finish the node
    auto emit_plane = [&](const float (&o)[2][2], float keep, float uown, int z, bool owned_plane, const RawNodes* W, int zpub) {
        const float left = lane_from_left(o[0][1], from_left, nfirst);
        xch[par][tid] = o[1][0] + lane_from_left(o[1][1], from_left, nfirst);
        if (W != nullptr) plane_publish(*W, zpub);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        float t = o[0][0] + left;
        if (ty > 0) t += xch[par][tid - 16];
        const bool st = owned_plane && owner && noderow_ok;
        if constexpr (E1G) ut_acc = st ? fmaf(t, uown, ut_acc) : ut_acc;      // before the Dirichlet rows are zeroed
        t *= keep;
        sq_acc = st ? fmaf(t, t, sq_acc) : sq_acc;
        pend_v = t * p.out_scale;
        pend_off = (unsigned)z * npl + out_row + (unsigned)x0;
        pend_st = st && sb.out != nullptr && x0 < p.nx;
        par ^= 1;
    };
    auto layer = [&](int ez, const PlaneN& L, const PlaneN& U, const RawNodes* W) {
        const bool own_layer = ez >= ez_own;
        const float cnt = (own_layer && owner) ? 1.f : 0.f;
        float o[2][2], fg[1] = {0.f};
        float tU[NGP][NGP], tX[NGP], tY[NGP], e1, e2;
        q1_layer_3d_w<NGP, false, HAS_F, UW>(TV, L.VU, U.VU, L.VX, U.VX, L.VY, U.VY, L.VN, U.VN, L.VF, U.VF, fg, cU, cX, cY, tU, tX, tY, e1, e2);
        if constexpr (E1G) {
            asm volatile("" : "+v"(e2));
        } else {
            asm volatile("" : "+v"(e1), "+v"(e2));
            e1_acc = fmaf(cnt * okf, e1, e1_acc);
        }
        e2_acc = fmaf(cnt * okf, e2, e2_acc);
        plane_transpose<NGP, float>(TV.b, okf, tU, tX, tY, o);
        __builtin_amdgcn_sched_barrier(0);
        emit_plane(o, L.keep, L.uown, ez, own_layer, W, ez + 2);
    };
    auto top_plane = [&](bool odd) {
        float o[2][2];
        plane_transpose<NGP, float>(TV.b, okf, cU, cX, cY, o);
        emit_plane(o, odd ? SB.keep : SA.keep, odd ? SB.uown : SA.uown, p.nz - 1, true, nullptr, 0);
    };

    if (lane < 9 && wave * 9 + lane < 33) {          // the constant components of the halo records (both parities): nu = 1, f = 0, keep = 1
        rec[0][halo_rec] = make_float4(0.f, 1.f, 0.f, 1.f);
        rec[1][halo_rec] = make_float4(0.f, 1.f, 0.f, 1.f);
    }
    __syncthreads();
#include "poisson3d_q1_march.inl"

    if constexpr (E1G) e1_acc = (ut_acc / p.T.esc + p.T.beta * e2_acc) / p.T.alpha;       // per-thread share of sum W nu |grad u|^2 (the identity holds for the total)
    if (p.want_sums) finish_sums(p, e1_acc, e2_acc, sq_acc, tid, 256, red, &last_flag, (double)p.T.esc);
}

#if DN_NGP == 2
// =============================================================================================================
// Fourth form (round 3): the node-owner form with TWO ELEMENTS PER THREAD along x, for the exact 2-point rule.  The node-owner kernel above
// is bound by instructions, and a third of them are per THREAD, not per element: the requests (8 vector-memory instructions per layer), the
// LDS records (4 reads, 2 writes), the hand-over (2 lane exchanges, slot write / read), the barrier, the Dirichlet selects, the store.  Here a
// thread owns the nodes x = nx0 + 2 tx, + 1 of row ny0 + ty (one 8-byte load per field and plane, one 8-byte store) and the two elements to
// their right; the tile is 32 x 16 elements (31 x 15 of them not shared with a neighbouring tile).  Records live in two LDS arrays, even and
// odd node columns, so that the three records a thread reads per node row are conflict-free b128 reads (lane stride 16 bytes).  The halo -- node
// row 16 (33 nodes) and node column 32 (16 nodes) -- is loaded 13 nodes per wave.  Needs an even nx (8-byte aligned pairs).
// =============================================================================================================
template <int FL>     // 3 waves per SIMD, the load-vector instantiations included (no staged forcing planes: 141-151 VGPRs with nu)
__global__ void __launch_bounds__(256, 3) poisson3d_q1n2_kernel(const PoissonParams p, const int chunks_x, const int tiles_y, const int strips_z) {
    constexpr int NGP = 2;
    constexpr bool UW = true;
    // LOADV: the forcing arrives as the assembled load vector (one value per node, used by the node's owner only: no staging, no element
    // arithmetic); F_ARR: the third array is read at all (it travels in the records' .z either way); HAS_F: nodal forcing, staged per element
    constexpr bool HAS_NU = (FL & FL3_NU) != 0, F_ARR = (FL & FL3_F) != 0, LOADV = F_ARR && (FL & FL3_LOAD) != 0, HAS_F = F_ARR && !LOADV;
    constexpr bool BC_U8C = (FL & FL3_BC_U8C) != 0, BOX = (FL & FL3_BOX) != 0;
    constexpr int NMASK = !BC_U8C ? 0 : ((FL & FL3_BC_ONE) ? 1 : 2);
    constexpr bool MASK_F32 = (FL & FL3_BC_F32) != 0;
    constexpr bool E1G = (FL & FL3_E1G) != 0;
    static_assert((FL & (FL3_FGP | FL3_BC)) == 0, "node-owner form: nodal forcing, constant-value conditions");
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int tid = ty * 16 + tx;
    const Strip3D wg = strip3d_decode(xcd_remap(blockIdx.x, gridDim.x), chunks_x, tiles_y, strips_z, p.strip_sel, p.nstrips, p.rows_per_strip, p.nelz);
    const int chunk = wg.chunk, tile = wg.tile, b = wg.b, ez_own = wg.ez_own, ez_begin = wg.ez_begin, ez_end = wg.ez_end;
    const int nx0 = chunk * 30, ny0 = tile * 15;               // first node of the tile (chunks overlap by one thread column = two elements)
    const int x0 = nx0 + 2 * tx, ey = ny0 + ty;                // the thread's first node == lower-left node of its first element
    const bool owner = !(chunk > 0 && tx == 0) && !(tile > 0 && ty == 0);
    const unsigned npl = (unsigned)(p.nx * p.ny);
    const int64_t nps = (int64_t)npl * p.nz;
    const SampleBases sb = sample_bases(p, b, nps);
    const bool noderow_ok = ey < p.ny;
    const float okf[2] = {(ey < p.nely && x0 < p.nelx) ? 1.f : 0.f, (ey < p.nely && x0 + 1 < p.nelx) ? 1.f : 0.f};
    const ElemTab& TV = p.T;

    __shared__ float4 recE[2][17][17];            // [plane parity][node row][even node column / 2] = {u after Dirichlet, nu, f, keep}
    __shared__ float4 recO[2][17][16];
    __shared__ float2 xch[2][256];
    __shared__ double red[2 * (256 / 64)];
    __shared__ int last_flag;
    if (blockIdx.x == 0u) fold_prev_sums(p, tid, 256, red);       // dn_poisson_args.fold_prev: close the evaluation before this one

    // own pair (clamped into the mesh: nx is even, so a pair is inside or outside as a whole) and the halo node this thread fetches
    const unsigned own_off = (unsigned)min(ey, p.ny - 1) * (unsigned)p.nx + (unsigned)min(x0, p.nx - 2);
    const int lane = tid & 63, wave = tid >> 6;
    // 49 halo nodes, 13 per wave, and ONE load instruction for their u, nu and f: lanes 0..12 fetch u, 13..25 nu, 26..38 f of the wave's 13 nodes
    // through per-lane 64-bit addresses (a vector-memory instruction costs a wave ~64 cycles of issue whatever its active lanes: three
    // instructions for 13 lanes each were a third of the kernel's vector-memory issue time); the other lanes repeat lane 38
    const int hgrp = min(lane / 13, 2), hsub = min(lane - 13 * hgrp, 12);
    const int hidx = min(wave * 13 + hsub, 48);
    const int hrow = hidx < 33 ? 16 : hidx - 33, hcol = hidx < 33 ? hidx : 32;
    const unsigned halo_off = (unsigned)min(ny0 + hrow, p.ny - 1) * (unsigned)p.nx + (unsigned)min(nx0 + hcol, p.nx - 1);
    const bool halo_lane = lane < 39 && wave * 13 + hsub < 49 && (hgrp == 0 || (hgrp == 1 ? HAS_NU : HAS_F));       // (the load vector is needed at owned nodes only: no halo)
    float* const halo_rec0 = reinterpret_cast<float*>((hcol & 1) ? &recO[0][hrow][hcol >> 1] : &recE[0][hrow][hcol >> 1]) + hgrp;      // component .x / .y / .z
    const unsigned halo_par_stride = 4u * ((hcol & 1) ? 17u * 16u : 17u * 17u);                                                        // floats
    const float* const halo_src = (hgrp == 1 && HAS_NU) ? sb.nu : ((hgrp == 2 && HAS_F) ? sb.f : sb.u);                               // per lane

    const MaskImages mi = mask_images(sb.mask[0], sb.mask[1]);
    // BOX: per condition the faces of the domain box it fixes (0: not a box condition).  In-plane part per node (this thread's pair, its halo
    // node), constant over the march; the two faces across the marched axis per plane (wave-uniform)
    const int bfaces[2] = {BOX && p.bc[0].kind == DN_MASK_BOX ? p.bc[0].box_faces : 0, BOX && p.bc[1].kind == DN_MASK_BOX ? p.bc[1].box_faces : 0};
    auto box_xy = [&](int k, int x, int y) {
        return ((bfaces[k] & DN_FACE_XLO) && x == 0) || ((bfaces[k] & DN_FACE_XHI) && x == p.nx - 1) || ((bfaces[k] & DN_FACE_YLO) && y == 0) ||
               ((bfaces[k] & DN_FACE_YHI) && y == p.ny - 1);
    };
    const bool bxy0[2] = {box_xy(0, x0, ey), box_xy(1, x0, ey)}, bxy1[2] = {box_xy(0, x0 + 1, ey), box_xy(1, x0 + 1, ey)};
    const bool bxyh[2] = {box_xy(0, nx0 + hcol, ny0 + hrow), box_xy(1, nx0 + hcol, ny0 + hrow)};

    struct RawNodes {
        float2 u, n, f;               // own pair
        float h;                      // halo node: u, nu or f by lane group
        PairMasks mk;
    };
    auto plane_request = [&](int zreq, RawNodes& W) {
        const unsigned zoff = (unsigned)min(zreq, p.nz - 1) * npl;
        const unsigned oo = zoff + own_off, oh = zoff + halo_off;
        W.u = ld_at<float2>(sb.u, oo);
        if constexpr (HAS_NU) W.n = ld_at<float2>(sb.nu, oo);
        if constexpr (F_ARR) W.f = ld_at<float2>(sb.f, oo);
        W.h = halo_src[oh];
        pair_masks_request<NMASK, MASK_F32>(mi, oo, oh, W.mk);
    };
    // img[j]: the node is set in the j-th LOADED mask image (NMASK == 1: the one image is whichever condition has it); box[k]: by condition k's faces.
    // The conditions are applied in their order (the reference's torch.where lines, e.g. IBN_3D.py:119-122)
    auto record = [&](float uu, float nn, float ff, const bool (&img)[2], const bool (&box)[2]) {
        float keep = 1.f;
        if constexpr (BC_U8C || BOX) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                bool s = false;
                if constexpr (NMASK == 2) s = mi.has[k] && img[k];
                if constexpr (NMASK == 1) s = mi.has[k] && img[0];
                if constexpr (BOX) s = s || box[k];
                uu = s ? p.bc[k].value : uu;
                keep = s ? 0.f : keep;
            }
        }
        return make_float4(uu, HAS_NU ? nn : 1.f, F_ARR ? ff : 0.f, keep);
    };
    auto plane_publish = [&](const RawNodes& W, int zpl) {
        bool s0[2], s1[2], sh[2];
        pair_masks_decode<NMASK, MASK_F32>(W.mk, s0, s1, sh);
        const int par = zpl & 1;
        bool b0[2] = {false, false}, b1[2] = {false, false}, bh[2] = {false, false};
        if constexpr (BOX) {
            const int zc = min(zpl, p.nz - 1);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const bool zf = ((bfaces[k] & DN_FACE_ZLO) && zc == 0) || ((bfaces[k] & DN_FACE_ZHI) && zc == p.nz - 1);
                b0[k] = bxy0[k] || zf; b1[k] = bxy1[k] || zf; bh[k] = bxyh[k] || zf;
            }
        }
        recE[par][ty][tx] = record(W.u.x, W.n.x, W.f.x, s0, b0);
        recO[par][ty][tx] = record(W.u.y, W.n.y, W.f.y, s1, b1);
        if (halo_lane) {
            float hv = W.h;
            if constexpr (BC_U8C || BOX) {
                if (hgrp == 0) hv = record(hv, 0.f, 0.f, sh, bh).x;
            }
            halo_rec0[par * halo_par_stride] = hv;       // (the .w of a halo record is never read; absent nu / f keep the 1 / 0 of the prologue)
        }
    };
    // From here on a value of type v2f holds the same quantity of the thread's two elements (.x: element at node column x0, .y: at x0 + 1) or
    // of its two nodes: the element arithmetic runs on packed fp32 instructions, one per pair.
    struct PlaneP { v2f VU[NGP][NGP], VX[NGP], VY[NGP], VN[NGP][NGP], VF[NGP][NGP]; };
    v2f ut_acc = 0.f;                             // E1G: sum of u * out over the owned nodes
    auto plane_gather = [&](int zpl, PlaneP& S) {
        const int par = zpl & 1;
        const float4 a0 = recE[par][ty][tx], a1 = recO[par][ty][tx], a2 = recE[par][ty][tx + 1];
        const float4 b0 = recE[par][ty + 1][tx], b1 = recO[par][ty + 1][tx], b2 = recE[par][ty + 1][tx + 1];
        stage_u3<NGP, v2f>(TV, v2f{a0.x, a1.x}, v2f{a1.x, a2.x}, v2f{b0.x, b1.x}, v2f{b1.x, b2.x}, S.VU, S.VX, S.VY);
        if constexpr (HAS_NU) stage_w3<NGP, UW, v2f>(TV, v2f{a0.y, a1.y}, v2f{a1.y, a2.y}, v2f{b0.y, b1.y}, v2f{b1.y, b2.y}, S.VN);
        if constexpr (HAS_F) stage_w3<NGP, UW, v2f>(TV, v2f{a0.z, a1.z}, v2f{a1.z, a2.z}, v2f{b0.z, b1.z}, v2f{b1.z, b2.z}, S.VF);
        __builtin_amdgcn_sched_barrier(0);
    };

    PlaneP SA, SB;
    v2f cU[NGP][NGP], cX[NGP], cY[NGP];
#pragma unroll
    for (int j = 0; j < NGP; ++j) {
        cX[j] = cY[j] = 0.f;
#pragma unroll
        for (int i = 0; i < NGP; ++i) {
            cU[j][i] = 0.f;
            SA.VN[j][i] = SB.VN[j][i] = 1.f;              // nu absent: the constant field 1 (unit weights)
            SA.VF[j][i] = SB.VF[j][i] = 0.f;
        }
    }

    v2f e1_acc2 = 0.f, e2_acc2 = 0.f, sq_acc2 = 0.f;
    const v2f okv = {okf[0], okf[1]};
    int par = 0;

    const unsigned out_row = (unsigned)ey * (unsigned)p.nx;
    const int from_left = (int)(((unsigned)tid - 1u) & 63u) << 2;
    const float nfirst = tx > 0 ? 1.f : 0.f;
    float2 pend_v = make_float2(0.f, 0.f);
    unsigned pend_off = 0u;
    bool pend_st = false;
    auto flush_store = [&]() {
        if (pend_st) st_at<float2>(sb.out, pend_off, pend_v);
        pend_st = false;
    };
    // o[node row][node column of the element]: contributions of the thread's two elements (.x, .y) to their 2 x 2 nodes in the plane being
    // finished.  The thread's node columns: c0 = o[.][0].x (+ the left thread's o[.][1].y), c1 = o[.][1].x + o[.][0].y; o[.][1].y goes right.
    auto emit_plane = [&](const v2f (&o)[2][2], int z, bool owned_plane, const RawNodes* W, int zpub) {
        // keep and (E1G) the value of the own node pair in the plane being finished: re-read from the thread's own records rather than carried in
        // eight registers through the layer (the kernel sits at its register cap).  The reads are issued BEFORE this call's publish overwrites the
        // records of the same parity (a wave's LDS accesses execute in order) and land under the barrier.
        const float4 own0 = recE[z & 1][ty][tx], own1 = recO[z & 1][ty][tx];
        const v2f keep = {own0.w, own1.w}, uown = {own0.x, own1.x};
        const v2f bown = {own0.z, own1.z};            // LOADV: the load vector at the own node pair
        const float left0 = lane_from_left(o[0][1].y, from_left, nfirst);
        xch[par][tid] = make_float2(o[1][0].x + lane_from_left(o[1][1].y, from_left, nfirst), o[1][1].x + o[1][0].y);
        if (W != nullptr) plane_publish(*W, zpub);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        v2f t = {o[0][0].x + left0, o[0][1].x + o[0][0].y};
        if (ty > 0) {
            const float2 up = xch[par][tid - 16];
            t += v2f{up.x, up.y};
        }
        const bool st = owned_plane && owner && noderow_ok;
        if constexpr (LOADV) {
            // out_a -= beta * wscale * b_a,  sum W f u = sum_a u_a b_a (u after the Dirichlet conditions): one FMA each per owned node.
            // Threads beyond the mesh hold a clamped duplicate of a valid pair: excluded.
            const bool inmesh = st && x0 < p.nx;
            t = inmesh ? vfma(TV.nbw, bown, t) : t;
            e2_acc2 = inmesh ? vfma(uown, bown, e2_acc2) : e2_acc2;
        }
        if constexpr (E1G) ut_acc = st ? vfma(t, uown, ut_acc) : ut_acc;      // before the Dirichlet rows are zeroed
        t *= keep;
        sq_acc2 = st ? vfma(t, t, sq_acc2) : sq_acc2;
        pend_v = make_float2(t.x * p.out_scale, t.y * p.out_scale);
        pend_off = (unsigned)z * npl + out_row + (unsigned)x0;
        pend_st = st && sb.out != nullptr && x0 < p.nx;
        par ^= 1;
    };
    auto layer = [&](int ez, const PlaneP& L, const PlaneP& U, const RawNodes* W) {
        const bool own_layer = ez >= ez_own;
        const v2f cnt = ((own_layer && owner) ? 1.f : 0.f) * okv;
        v2f o[2][2], tU[NGP][NGP], tX[NGP], tY[NGP], e1, e2;
        float fg[1] = {0.f};
        q1_layer_3d_w<NGP, false, HAS_F, UW, v2f>(TV, L.VU, U.VU, L.VX, U.VX, L.VY, U.VY, L.VN, U.VN, L.VF, U.VF, fg, cU, cX, cY, tU, tX, tY, e1, e2);
        if constexpr (E1G) {
            asm volatile("" : "+v"(e2));
        } else {
            asm volatile("" : "+v"(e1), "+v"(e2));
            e1_acc2 = vfma(cnt, e1, e1_acc2);
        }
        e2_acc2 = vfma(cnt, e2, e2_acc2);
        plane_transpose<NGP, v2f>(TV.b, okv, tU, tX, tY, o);
        __builtin_amdgcn_sched_barrier(0);
        emit_plane(o, ez, own_layer, W, ez + 2);
    };
    auto top_plane = [&](bool) {
        v2f o[2][2];
        plane_transpose<NGP, v2f>(TV.b, okv, cU, cX, cY, o);
        emit_plane(o, p.nz - 1, true, nullptr, 0);
    };

    if (lane < 13 && wave * 13 + lane < 49) {          // the constant components of the halo records (both parities): nu = 1, f = 0, keep = 1
        float4* const r0 = (hcol & 1) ? &recO[0][hrow][hcol >> 1] : &recE[0][hrow][hcol >> 1];
        const unsigned st4 = (hcol & 1) ? 17u * 16u : 17u * 17u;
        r0[0] = make_float4(0.f, 1.f, 0.f, 1.f);
        r0[st4] = make_float4(0.f, 1.f, 0.f, 1.f);
    }
    __syncthreads();
#include "poisson3d_q1_march.inl"

    float e1_acc = e1_acc2.x + e1_acc2.y;
    const float e2_acc = e2_acc2.x + e2_acc2.y, sq_acc = sq_acc2.x + sq_acc2.y;
    if constexpr (E1G) e1_acc = ((ut_acc.x + ut_acc.y) / p.T.esc + p.T.beta * e2_acc) / p.T.alpha;
    if (p.want_sums) finish_sums(p, e1_acc, e2_acc, sq_acc, tid, 256, red, &last_flag, (double)p.T.esc);
}
#endif

// ---- dispatch ---------------------------------------------------------------------------------------------
// unit: the exact 2-point rule's weights, all 1 (UW kernels exist for 2 points only)
template <int NGP>
static bool unit_weights(const PoissonParams& pp) {
    bool unit = NGP == 2;
    for (int i = 0; i < NGP; ++i) unit = unit && pp.T.w[i] == 1.0f;
    return unit;
}

// node-owner form (every node requested once) with FL's mask images, or (one) with exactly one of them
template <int NGP, int FL, bool UW>
static void launch3_n1(const PoissonParams& pp, const Geom3D& g, const dim3& grid, bool one, hipStream_t s) {
    constexpr int FL1 = (FL & FL3_BC_U8C) ? (FL | FL3_BC_ONE) : FL;
    const dim3 block(16, 16);
    if (one) hipLaunchKernelGGL((poisson3d_q1n_kernel<NGP, FL1, UW>), grid, block, 0, s, pp, g.chunks, g.tiles, g.strips);
    else hipLaunchKernelGGL((poisson3d_q1n_kernel<NGP, FL, UW>), grid, block, 0, s, pp, g.chunks, g.tiles, g.strips);
}

template <int NGP, int FL>
static void launch3_one(const PoissonParams& pp, const Geom3D& g, int family, int batch, hipStream_t s) {
    const dim3 grid((unsigned)((long long)g.chunks * g.tiles * g.strips * batch)), block(g.TX, g.TY);
    const bool unit = unit_weights<NGP>(pp);
    if constexpr ((FL & (FL3_FGP | FL3_BC)) == 0) {
        if (family == DN_POISSON_3D_Q1_N1) {
            const bool one = (FL & FL3_BC_U8C) && ((pp.bc[0].mask != nullptr) != (pp.bc[1].mask != nullptr));
            if constexpr (NGP == 2) {
                if (unit) {
                    // energy from the nodal values (FL3_E1G) whenever the launch has a stiffness part and sums are wanted
                    if (pp.T.alpha != 0.f && pp.want_sums && config(CFG_Q1_3D_E1SUM) == nullptr) launch3_n1<NGP, FL | FL3_E1G, true>(pp, g, grid, one, s);
                    else launch3_n1<NGP, FL, true>(pp, g, grid, one, s);
                    return;
                }
            }
            launch3_n1<NGP, FL, false>(pp, g, grid, one, s);
            return;
        }
    }
    const bool t16 = family == DN_POISSON_3D_Q1_T16;          // 16-wide tiles: lane-exchange hand-over, paired loads
#define DN_W3(UW, T16) hipLaunchKernelGGL((poisson3d_q1w_kernel<NGP, FL, UW, T16>), grid, block, 0, s, pp, g.chunks, g.tiles, g.strips)
    if constexpr (NGP == 2) {
        if (unit) {
            if (t16) DN_W3(true, true);
            else DN_W3(true, false);
            return;
        }
    }
    if (t16) DN_W3(false, true);
    else DN_W3(false, false);
#undef DN_W3
}

// node-owner form with fp32 mask images (constant values); only instantiated for nodal / absent forcing
template <int NGP, int FL>
static void launch3_f32n(const PoissonParams& pp, const Geom3D& g, int family, int batch, hipStream_t s) {
    if constexpr ((FL & FL3_FGP) == 0) {
        const dim3 grid((unsigned)((long long)g.chunks * g.tiles * g.strips * batch));
        const bool one = (pp.bc[0].mask != nullptr) != (pp.bc[1].mask != nullptr);
        if constexpr (NGP == 2) {
            if (unit_weights<NGP>(pp)) {
                launch3_n1<NGP, FL | FL3_BC_U8C | FL3_BC_F32, true>(pp, g, grid, one, s);
                return;
            }
        }
        launch3_n1<NGP, FL | FL3_BC_U8C | FL3_BC_F32, false>(pp, g, grid, one, s);
    } else {
        launch3_one<NGP, FL | FL3_BC>(pp, g, family, batch, s);
    }
}

template <int NGP>
static void launch3_flags(const PoissonParams& pp, const Geom3D& g, int family, int batch, hipStream_t s) {
    const int f = pp.fgp ? 2 : (pp.f ? 1 : 0);
    const bool bc = pp.bc[0].mask || pp.bc[1].mask;
    bool u8c = bc, f32c = bc;                        // all conditions uint8 / all fp32 images, constant values
    for (int k = 0; k < 2; ++k) {
        if (pp.bc[k].mask && (!pp.bc[k].mask_is_u8 || pp.bc[k].field)) u8c = false;
        if (pp.bc[k].mask && (pp.bc[k].mask_is_u8 || pp.bc[k].field)) f32c = false;
    }
    // fp32 images with constant values (the reference's masks): the node-owner form reads them as one dword per node; everything else
    // with fp32 masks or value fields goes through the generic form of the T16 kernel
    const bool f32n = f32c && family == DN_POISSON_3D_Q1_N1;
#define DN_L3(FLAGS)                                                           \
    (!bc ? launch3_one<NGP, (FLAGS)>(pp, g, family, batch, s)                    \
         : u8c ? launch3_one<NGP, (FLAGS) | FL3_BC_U8C>(pp, g, family, batch, s) \
         : f32n ? launch3_f32n<NGP, (FLAGS)>(pp, g, family, batch, s)            \
               : launch3_one<NGP, (FLAGS) | FL3_BC>(pp, g, family, batch, s))
    if (pp.nu) {
        if (f == 0) DN_L3(FL3_NU);
        else if (f == 1) DN_L3(FL3_NU | FL3_F);
        else DN_L3(FL3_NU | FL3_FGP);
    } else {
        if (f == 0) DN_L3(0);
        else if (f == 1) DN_L3(FL3_F);
        else DN_L3(FL3_FGP);
    }
#undef DN_L3
}

#if DN_NGP == 2
template <int FLB>
static void launch3_n2_bc(const PoissonParams& pp, const dim3& grid, const Geom3D& g, hipStream_t s) {
    launch_mask_form(pp.bc, [&](auto form) {
        hipLaunchKernelGGL((poisson3d_q1n2_kernel<FLB | decltype(form)::value>), grid, dim3(16, 16), 0, s, pp, g.chunks, g.tiles, g.strips);
    });
}

static int launch3_n2(const PoissonParams& pp, const Geom3D& g, int batch, hipStream_t s) {
    const dim3 grid((unsigned)((long long)g.chunks * g.tiles * g.strips * batch));
    // energy from the nodal values (FL3_E1G) whenever the launch has a stiffness part and sums are wanted
    const bool e1g = pp.T.alpha != 0.f && pp.want_sums && config(CFG_Q1_3D_E1SUM) == nullptr;
    const int sel = (pp.nu ? 1 : 0) | (pp.f ? 2 : 0) | (e1g ? 4 : 0);
    if (pp.f && pp.f_is_load) {                    // the forcing as the assembled load vector (dn_poisson_args.f_is_load)
        switch (sel) {
            case 2: launch3_n2_bc<FL3_F | FL3_LOAD>(pp, grid, g, s); break;
            case 3: launch3_n2_bc<FL3_NU | FL3_F | FL3_LOAD>(pp, grid, g, s); break;
            case 6: launch3_n2_bc<FL3_F | FL3_LOAD | FL3_E1G>(pp, grid, g, s); break;
            default: launch3_n2_bc<FL3_NU | FL3_F | FL3_LOAD | FL3_E1G>(pp, grid, g, s); break;
        }
        return 0;
    }
    switch (sel) {
        case 0: launch3_n2_bc<0>(pp, grid, g, s); break;
        case 1: launch3_n2_bc<FL3_NU>(pp, grid, g, s); break;
        case 2: launch3_n2_bc<FL3_F>(pp, grid, g, s); break;
        case 3: launch3_n2_bc<FL3_NU | FL3_F>(pp, grid, g, s); break;
        case 4: launch3_n2_bc<FL3_E1G>(pp, grid, g, s); break;
        case 5: launch3_n2_bc<FL3_NU | FL3_E1G>(pp, grid, g, s); break;
        case 6: launch3_n2_bc<FL3_F | FL3_E1G>(pp, grid, g, s); break;
        default: launch3_n2_bc<FL3_NU | FL3_F | FL3_E1G>(pp, grid, g, s); break;
    }
    return 0;
}
#endif

#define DN_CAT2(a, b) a##b
#define DN_CAT(a, b) DN_CAT2(a, b)
int DN_CAT(launch_poisson3d_q1_g, DN_NGP)(const PoissonParams& pp, const Geom3D& g, int family, int batch, bool vec, hipStream_t s) {
    if (pp.f && pp.f_is_load && !(DN_NGP == 2 && g.E == 2 && g.TX == 16 && g.TY == 16)) return DN_E_UNSUPPORTED;      // load vectors: two-element node-owner form only
    if (g.E == 1) { launch3_flags<DN_NGP>(pp, g, family, batch, s); return 0; }
#if DN_NGP == 2
    if (g.E == 2 && g.TX == 16 && g.TY == 16) {
        // node-owner forms, two elements per thread (poisson_choose checked their preconditions): closed form in z (poisson3d_q1_cf.hip) or marching
        if (family == DN_POISSON_3D_Q1_CFZ) return launch_poisson3d_q1_cf(pp, g, batch, s);
        return launch3_n2(pp, g, batch, s);
    }
#endif
    return DN_E_UNSUPPORTED;
}

}  // namespace dn
