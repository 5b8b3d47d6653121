// What the 3-D Q1 fused Poisson kernels share (poisson3d_q1.inl: poisson3d_q1w_kernel, poisson3d_q1n_kernel, poisson3d_q1n2_kernel;
// poisson3d_q1_cf.hip: poisson3d_q1_cf_kernel): the workgroup's place in the launch, the lane exchange, the adjoint of the in-plane stage, the
// mask images, and the raw mask words of the tile of node PAIRS of the two two-element kernels.
// Every device helper here sees ints, floats, bools and pointers only, never the kernel's parameter block: a helper that reads PoissonParams
// makes the compiler split the block into SGPRs again at kernel entry (profiles/flow2d_refactor.txt, profiles/owner_march_refactor.txt).
#pragma once
#include <type_traits>

#include "poisson_common.h"

namespace dn {

// Compile-time form of a kernel.  poisson3d_q1w_kernel: NU, F, FGP, BC, BC_U8C; the node-owner kernels: NU, F, BC_U8C, BC_ONE, BC_F32 and
// (two elements per thread, marching and closed form) LOAD, BOX; FL3_E1G: the marching node-owner kernels only.
//   FL3_BC_U8C: constant-value conditions held as mask images -- uint8, or with FL3_BC_F32 fp32 (> 0.5, the reference's format); FL3_BC_ONE:
//     exactly one image;  FL3_BC: any other kind of mask or value fields (poisson3d_q1w_kernel)
//   FL3_LOAD (with FL3_F): `f` holds the ASSEMBLED load vector b_a = sum_e sum_g W_g N_a f_g (dn_poisson_args.f_is_load) -- one FMA per node
//     instead of the element's forcing arithmetic
//   FL3_BOX: at least one condition is given as faces of the domain box (DN_MASK_BOX): no array, no load
enum : int { FL3_NU = 1, FL3_F = 2, FL3_FGP = 4, FL3_BC = 8, FL3_BC_U8C = 16, FL3_BC_ONE = 32, FL3_E1G = 64, FL3_BC_F32 = 128, FL3_LOAD = 256, FL3_BOX = 512 };

// A workgroup's place in the 1-D launch (logical order: chunk fastest, then tile, strip, sample; `lid` after xcd_remap) and the element layers of its
// strip: it owns [ez_own, ez_end) and, above the first strip, recomputes the layer below for its first node plane.
struct Strip3D { int chunk, tile, strip, b, ez_own, ez_begin, ez_end; };
__device__ __forceinline__ Strip3D strip3d_decode(unsigned lid, int chunks_x, int tiles_y, int strips_z, int strip_sel, int nstrips, int R, int nelz) {
    Strip3D s;
    s.chunk = (int)(lid % (unsigned)chunks_x);
    lid /= (unsigned)chunks_x;
    s.tile = (int)(lid % (unsigned)tiles_y);
    lid /= (unsigned)tiles_y;
    s.strip = selected_strip(strip_sel, nstrips, (int)(lid % (unsigned)strips_z));
    s.b = (int)(lid / (unsigned)strips_z);
    s.ez_own = s.strip * R;
    s.ez_begin = s.ez_own > 0 ? s.ez_own - 1 : 0;
    s.ez_end = min(s.ez_own + R, nelz);
    return s;
}

// lane l <- lane l - 1 inside each row of 16 lanes, 0 for the first lane.  NOT a DPP move: on gfx950 every DPP / SDWA / v_readlane
// instruction costs a SIMD ~33 cycles (about 14 plain VALU instructions) as soon as two or more waves share it, while a
// ds_bpermute_b32 / ds_swizzle_b32 costs ~3 (tools/micro/valu_mem.hip, profiles/r2_valu_mem.txt).  `from` is the byte address of the
// source lane ((lane - 1) & 63) * 4, `nf` is 0 for the first lane of a row and 1 elsewhere.
__device__ __forceinline__ float lane_from_left(float v, int from, float nf) {
    return nf * __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(from, __builtin_bit_cast(int, v)));
}

// adjoint of stage_u3: cotangents of one plane's stage values -> contributions o[node row][node column] to the element's 2 x 2 nodes, times
// `ok` (0 for an element beyond the mesh).  b: ElemTab::b.  V = float, or v2f: the thread's two elements at once.  ACC: the contributions are
// ADDED to o (poisson3d_q1w_kernel, on zeros, as it always has: the two forms can differ in the sign of a zero)
template <int NGP, typename V, bool ACC = false>
__device__ __forceinline__ void plane_transpose(const float (&b)[4][4], V ok, const V (&tU)[NGP][NGP], const V (&tX)[NGP], const V (&tY)[NGP], V (&o)[2][2]) {
    V s0 = 0.f, t0 = 0.f, s1 = 0.f, t1 = 0.f;
#pragma unroll
    for (int i = 0; i < NGP; ++i) {
        V sv = 0.f, t = 0.f;
#pragma unroll
        for (int j = 0; j < NGP; ++j) { sv += tU[j][i]; t = vfma(b[j][1], tU[j][i], t); }
        const V c1 = t + tY[i], c0 = sv - c1;
        s0 += c0; t0 = vfma(b[i][1], c0, t0);
        s1 += c1; t1 = vfma(b[i][1], c1, t1);
    }
    V sX = 0.f, d1 = 0.f;
#pragma unroll
    for (int j = 0; j < NGP; ++j) { sX += tX[j]; d1 = vfma(b[j][1], tX[j], d1); }
    const V g01 = t0 + (sX - d1), g11 = t1 + d1;
    if constexpr (ACC) {
        o[0][1] = vfma(ok, g01, o[0][1]); o[0][0] = vfma(ok, s0 - g01, o[0][0]);
        o[1][1] = vfma(ok, g11, o[1][1]); o[1][0] = vfma(ok, s1 - g11, o[1][0]);
    } else {
        o[0][1] = ok * g01; o[0][0] = ok * (s0 - g01);
        o[1][1] = ok * g11; o[1][0] = ok * (s1 - g11);
    }
}

// The two mask images of a sample as byte and as fp32 pointers.  An absent condition re-reads the other one and is ignored: both slots are
// always loaded, since a load inside a wave-uniform branch makes the compiler wait vmcnt(0) at the end of the branch, which serialises every
// load of the plane behind it.
struct MaskImages {
    bool has[2];
    const uint8_t* m8[2];
    const float* m32[2];
};
__device__ __forceinline__ MaskImages mask_images(const void* m0, const void* m1) {
    MaskImages mi;
    mi.has[0] = m0 != nullptr; mi.has[1] = m1 != nullptr;
    mi.m8[0] = reinterpret_cast<const uint8_t*>(mi.has[0] ? m0 : m1);
    mi.m8[1] = reinterpret_cast<const uint8_t*>(mi.has[1] ? m1 : m0);
    mi.m32[0] = reinterpret_cast<const float*>(mi.m8[0]); mi.m32[1] = reinterpret_cast<const float*>(mi.m8[1]);
    return mi;
}

// ---- the tile of node pairs (poisson3d_q1n2_kernel, poisson3d_q1_cf_kernel) ----------------------------------------------------------------
// (The tile origin, the halo assignment, the box-face tests and the in-order application of the conditions stay spelled out in the two kernels:
// profiles/poisson3d_refactor.txt.)
// Raw mask words of one plane, as loaded (NMASK images, uint8 or F32): the own pair (two bytes / two floats) and the halo node
struct PairMasks {
    uint16_t m[2];
    float2 mf[2];
    uint8_t hm[2];
    float hmf[2];
};
template <int NMASK, bool F32>
__device__ __forceinline__ void pair_masks_request(const MaskImages& mi, unsigned own, unsigned halo, PairMasks& r) {
#pragma unroll
    for (int k = 0; k < NMASK; ++k) {
        if constexpr (F32) { r.mf[k] = ld_at<float2>(mi.m32[k], own); r.hmf[k] = ld_at<float>(mi.m32[k], halo); }
        else { r.m[k] = ld_at<uint16_t>(mi.m8[k], own); r.hm[k] = ld_at<uint8_t>(mi.m8[k], halo); }
    }
}
// -> the node is set in the k-th LOADED image: s0 / s1 the own pair, sh the halo node (false for an image that is not loaded)
template <int NMASK, bool F32>
__device__ __forceinline__ void pair_masks_decode(const PairMasks& r, bool (&s0)[2], bool (&s1)[2], bool (&sh)[2]) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        s0[k] = s1[k] = sh[k] = false;
        if (k < NMASK) {
            if constexpr (F32) { s0[k] = r.mf[k].x > 0.5f; s1[k] = r.mf[k].y > 0.5f; sh[k] = r.hmf[k] > 0.5f; }
            else { s0[k] = (r.m[k] & 0xffu) != 0; s1[k] = (r.m[k] >> 8) != 0; sh[k] = r.hm[k] != 0; }
        }
    }
}

// Host: the mask form of a launch of the two-element kernels, handed to `launch` as a compile-time flag set (std::integral_constant): none, one
// or two images, uint8 or fp32, box faces alone or beside ONE image
template <class Launch>
static void launch_mask_form(const DirichletDev (&bc)[2], Launch&& launch) {
    const bool any = bc[0].mask || bc[1].mask;
    const bool one = (bc[0].mask != nullptr) != (bc[1].mask != nullptr);
    const bool f32 = (bc[0].mask && !bc[0].mask_is_u8) || (bc[1].mask && !bc[1].mask_is_u8);
    const bool box = bc[0].kind == DN_MASK_BOX || bc[1].kind == DN_MASK_BOX;
#define DN_FORM(FLAGS) launch(std::integral_constant<int, (FLAGS)>{})
    if (!any) { if (box) DN_FORM(FL3_BOX); else DN_FORM(0); }
    else if (box && !f32) DN_FORM(FL3_BOX | FL3_BC_U8C | FL3_BC_ONE);
    else if (box) DN_FORM(FL3_BOX | FL3_BC_U8C | FL3_BC_F32 | FL3_BC_ONE);
    else if (!f32 && one) DN_FORM(FL3_BC_U8C | FL3_BC_ONE);
    else if (!f32) DN_FORM(FL3_BC_U8C);
    else if (one) DN_FORM(FL3_BC_U8C | FL3_BC_F32 | FL3_BC_ONE);
    else DN_FORM(FL3_BC_U8C | FL3_BC_F32);
#undef DN_FORM
}

}  // namespace dn
