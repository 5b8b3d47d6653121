// Per-element arithmetic of the fused Poisson operator (energy density, its gradient / the weak-form
// residual) for one structured Q_P element, evaluated entirely in registers.
//
// What the reference does per element and Gauss point with dense nd tables
// (DiffNet/DiffNetFEM.py:196-227, 405-453 tables; IBN_2D.py:123-131, 12_klsum.py:96-122 use) is done
// here by sum factorisation: the 1-D basis tables are applied axis by axis.  For Q1 the 1-D
// basis is a lerp, phi(xi) = (1-b, b) with b = (1+xi)/2 and phi' = (-1/2, +1/2), so every 1-D
// contraction is one subtraction plus one FMA per Gauss point and the derivative is the
// difference itself; that specialisation is what keeps the kernel near the HBM roofline
// instead of the VALU roofline.
//
// nu and f are always interpolated from nodal values (an absent nu is the constant field 1, an
// absent f the constant 0: exact under interpolation), so the element code has no runtime flags;
// FGP selects forcing given directly at the Gauss points (e8_2d_poisson_mms.py:46).
//
// Conventions: W_g = w[jg] * wx[ig] (* w[kg]); the returned energy parts are
//   e1 = sum_g W_g nu_g |grad u|^2_g      (caller multiplies by c)
//   e2 = sum_g W_g f_g u_g
// and the nodal contributions are g_a = sum_g W_g ( alpha nu_g gradN_a.grad u_g - beta N_a f_g ).
#pragma once
#include "dn_common.h"

namespace dn {

// Value types of the element arithmetic: float, or v2f = two independent elements in the halves of a 64-bit register pair.  On gfx950 a
// packed fp32 instruction (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) costs a SIMD ~3.4 cycles per wave whatever its operands, a plain
// one 2.9 (registers only) to 4.0 (SGPR operand) -- per element-operation 1.7 against ~3.2 at this code's operand mix
// (tools/micro/valu_pk.hip, profiles/r3_valu_pk.txt).  SGPR table entries broadcast into both halves through op_sel, for free.
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float vfma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ v2f vfma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f vfma(float a, v2f b, v2f c) { return __builtin_elementwise_fma((v2f)(a), b, c); }

// Kernel-argument resident (SGPR) tables: everything wave-uniform the element code needs.
struct ElemTab {
    float b[4][4];       // b[ig][ib]  = phi_ib(xi_ig)
    float dx[4][4];      // dbasis[ig][ib] * 2/hx   (generic-degree path)
    float dy[4][4];
    float dz[4][4];
    float w[4];          // 1-D Gauss weights
    float wx[4];         // w[ig] * wscale (the x axis carries the Jacobian / user scale)
    float w2[4][4];      // w2[jg][ig] = w[jg] * wx[ig]
    float hs[3];         // Q1 path: 0.5 * 2/h_d = 1/h_d
    float ahs[3];        // alpha * hs[d]
    float alpha, beta, c;
    // Q1 marching kernels: moments of the 1-D rule against the lerp weight b = phi_1(xi):
    //   m[r] = sum_g w[g] * b[g]^r  (r = 0,1,2);  kx[r][ig] = wx[ig] * m[r]
    float m[4];          // m[r] = sum_g w[g] * b[g]^r, r = 0..3
    float mxs[4];        // m[r] * wscale (the x axis carries the Jacobian / user scale): closed-form 2-D Q1 kernel
    float kx[3][4];
    float q1c[4];        // alpha*hs0^2, alpha*hs1^2, hs0^2, hs1^2  (2-D Q1 layer: derivative scales applied once per element)
    // 3-D Q1 marching kernels (q1_layer_3d_w): the in-plane weights live in the staged coefficient planes, the
    // user scale (wscale) in kap[] and in the final energy scale, the 1/h factors are applied once per element.
    float wb[4];         // w[g] * b[g]           (pure 1-D weights: no wscale)
    float kap[3];        // alpha * wscale * hs[d]^2   cotangent scale of direction d
    float hs2[3];        // hs[d]^2                    energy scale of direction d (wscale is applied in finish_sums)
    float m01, m12;      // m[0] - m[1], m[1] - m[2]
    float esc;           // wscale: factor of both energy sums of the second-form kernel (1 for the other kernels)
    float nbw;           // -beta * wscale
    // closed-form 2-D Q1 kernel: the 1-D element mass matrix [[c00, c01], [c01, c11]] = sum_g w_g [(1-b)^2, b(1-b); b(1-b), b^2] of the
    // rule (from its moments, in double): the forcing term is (mass_x (x) mass_y) f, applied axis by axis (x carries wscale)
    float q1mx[3], q1my[3];   // c00, c01, c11
    // closed-form 2-D Q1 kernel, row-staged stiffness element (q1cf_elem below).  With r_rs = sum_g w_g (1 - b_g)^r b_g^s (r + s = 3) of the 1-D rule, in double:
    float q1xm[4];       // hs0^2 (r30, r21, r12, r03): x-derivative term (its nu x-moments pn carry wscale)
    float q1ym[4];       // hs1^2 wscale (r30, r21, r12, r03): y-derivative term
    float q1px[2];       // wscale (m0 - m1, m1): pn[e] = q1px[0] n[e] + q1px[1] n[e + 1]
    float q1sy[2];       // (m0 - m1, m1): y-moment of nu per node, S[n] = q1sy[0] n_L[n] + q1sy[1] n_U[n]
};

// ---------------------------------------------------------------------------------------------
// 2-D element.  u/nu/f: nodal values [jb][ib]; fg: forcing at Gauss points [jg*NGP+ig] (FGP).
// ---------------------------------------------------------------------------------------------
template <int P, int NGP, bool FGP>
__device__ __forceinline__ void elem2d(const ElemTab& T, const float (&u)[P + 1][P + 1], const float (&nu)[P + 1][P + 1],
                                       const float (&f)[P + 1][P + 1], const float* fg, float (&g)[P + 1][P + 1],
                                       float& e1, float& e2) {
    constexpr int NB = P + 1;
    float a1 = 0.f, a2 = 0.f;
    static_assert(P >= 2, "Q1 elements run through the marching kernels (q1_layer_2d / q1_layer_3d_w)");
    // Table-driven sum factorisation, one x-Gauss point at a time: x-stage of u / nu / f for that point (per node row),
    // its NGP y-points (energy density, cotangents, y-transpose), then the x-transpose of that point straight into g.
    // The live set is one point's stage values and cotangents instead of all points'.
#pragma unroll
    for (int jb = 0; jb < NB; ++jb)
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) g[jb][ib] = 0.f;
#pragma unroll
    for (int ig = 0; ig < NGP; ++ig) {
        float tv[NB], td[NB], tn[NB], tf[NB], rv[NB], rd[NB];
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
            float a = 0.f, d = 0.f, n = 0.f, q = 0.f;
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) {
                a = fmaf(T.b[ig][ib], u[jb][ib], a);
                d = fmaf(T.dx[ig][ib], u[jb][ib], d);
                n = fmaf(T.b[ig][ib], nu[jb][ib], n);
                if constexpr (!FGP) q = fmaf(T.b[ig][ib], f[jb][ib], q);
            }
            tv[jb] = a; td[jb] = d; tn[jb] = n; tf[jb] = q; rv[jb] = 0.f; rd[jb] = 0.f;
        }
#pragma unroll
        for (int jg = 0; jg < NGP; ++jg) {
            float val = 0.f, ux = 0.f, uy = 0.f, nuv = 0.f, fv = 0.f;
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
                val = fmaf(T.b[jg][jb], tv[jb], val);
                ux = fmaf(T.b[jg][jb], td[jb], ux);
                uy = fmaf(T.dy[jg][jb], tv[jb], uy);
                nuv = fmaf(T.b[jg][jb], tn[jb], nuv);
                if constexpr (!FGP) fv = fmaf(T.b[jg][jb], tf[jb], fv);
            }
            if constexpr (FGP) fv = fg[jg * NGP + ig];
            const float Wn = T.w2[jg][ig] * nuv, Wf = T.w2[jg][ig] * fv;
            a1 = fmaf(Wn, ux * ux + uy * uy, a1);
            a2 = fmaf(Wf, val, a2);
            const float qx = T.alpha * Wn * ux, qy = T.alpha * Wn * uy, qv = -T.beta * Wf;
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
                rv[jb] = fmaf(T.b[jg][jb], qv, rv[jb]);
                rv[jb] = fmaf(T.dy[jg][jb], qy, rv[jb]);
                rd[jb] = fmaf(T.b[jg][jb], qx, rd[jb]);
            }
        }
#pragma unroll
        for (int jb = 0; jb < NB; ++jb)
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) {
                g[jb][ib] = fmaf(T.b[ig][ib], rv[jb], g[jb][ib]);
                g[jb][ib] = fmaf(T.dx[ig][ib], rd[jb], g[jb][ib]);
            }
    }
    e1 = a1;
    e2 = a2;
}

// ---------------------------------------------------------------------------------------------
// 2-D Q1, marching form.  One element between node rows j (suffix 0) and j+1 (suffix 1), given the
// x-stage values of both rows at the element's x-Gauss points:
//   TU[ig] = lerp_x(u)(xi_ig), DX = u[e+1]-u[e];  TN, TF likewise for nu and f.
// Because nu, f and u are bilinear and the rule is a tensor product, every sum over the y-Gauss points
// collapses onto the three moments m[0..2] of the 1-D rule (ElemTab), so the work is O(NGP), not O(NGP^2).
// Outputs: cotangents of the x-stage values of both rows (ct0/ct1 for TU, cdx0/cdx1 for DX) -- the caller
// adds the carried cotangent of the shared row and applies the x-stage transpose once per row -- and the
// two energy parts (see the conventions at the top of this file).
// ---------------------------------------------------------------------------------------------
template <int NGP, bool FGP>
__device__ __forceinline__ void q1_layer_2d(const ElemTab& T, const float (&TU0)[NGP], const float (&TU1)[NGP], const float DX0,
                                            const float DX1, const float (&TN0)[NGP], const float (&TN1)[NGP],
                                            const float (&TF0)[NGP], const float (&TF1)[NGP], const float* fg,
                                            float (&ct0)[NGP], float (&ct1)[NGP], float& cdx0, float& cdx1, float& e1,
                                            float& e2) {
    // The 1/h factors of the derivatives are applied once per element (q1c[]) instead of once per Gauss point:
    //   e1 = hs0^2 * sum_jg w Qx' r_jg^2 + hs1^2 * sum_ig Qy d_ig^2,   r = raw x-difference lerp, d = raw y-difference
    float a1x = 0.f, a1y = 0.f, a2 = 0.f;
    // nu moments along x
    float S0 = 0.f, S1 = 0.f, dyn[NGP];
#pragma unroll
    for (int i = 0; i < NGP; ++i) {
        dyn[i] = TN1[i] - TN0[i];
        S0 = fmaf(T.wx[i], TN0[i], S0);
        S1 = fmaf(T.wx[i], dyn[i], S1);
    }
    // x-derivative depends on the y-Gauss index only
    const float ddx = DX1 - DX0;
    float c1s = 0.f, css = 0.f;
#pragma unroll
    for (int jg = 0; jg < NGP; ++jg) {
        const float r = fmaf(T.b[jg][1], ddx, DX0);
        const float t = fmaf(T.b[jg][1], S1, S0) * r;          // (nu-moment) * raw derivative
        a1x = fmaf(T.w[jg] * t, r, a1x);
        const float cx = T.w[jg] * t;
        css += cx;
        c1s = fmaf(T.b[jg][1], cx, c1s);
    }
    const float kx = T.q1c[0];                                   // alpha * hs0^2
    cdx1 = kx * c1s;
    cdx0 = kx * css - cdx1;
    const float nb = -T.beta, ky = T.q1c[1];                     // alpha * hs1^2
#pragma unroll
    for (int ig = 0; ig < NGP; ++ig) {
        const float dyv = TU1[ig] - TU0[ig];
        const float t = fmaf(T.kx[1][ig], dyn[ig], T.kx[0][ig] * TN0[ig]) * dyv;
        a1y = fmaf(t, dyv, a1y);
        float cs, c1;
        if constexpr (FGP) {
            cs = 0.f; c1 = 0.f;
#pragma unroll
            for (int jg = 0; jg < NGP; ++jg) {
                const float wf = T.w2[jg][ig] * fg[jg * NGP + ig];
                cs += wf;
                c1 = fmaf(T.b[jg][1], wf, c1);
            }
        } else {
            const float dyf = TF1[ig] - TF0[ig];
            cs = fmaf(T.kx[1][ig], dyf, T.kx[0][ig] * TF0[ig]);
            c1 = fmaf(T.kx[2][ig], dyf, T.kx[1][ig] * TF0[ig]);
        }
        a2 = fmaf(cs, TU0[ig], a2);
        a2 = fmaf(c1, dyv, a2);
        ct1[ig] = fmaf(nb, c1, ky * t);
        ct0[ig] = fmaf(nb, cs, -ct1[ig]);
    }
    e1 = fmaf(T.q1c[2], a1x, T.q1c[3] * a1y);                    // hs0^2 * a1x + hs1^2 * a1y
    e2 = a2;
}

// ---------------------------------------------------------------------------------------------
// 2-D Q1, closed form, symmetric in the lower (L) and upper (U) node row of the layer (poisson2d_q1_cf.hip).  Staged once per node
// row and element:  du[e] = u[e + 1] - u[e]  and the x-moment of nu  pn[e] = sum_i wx_i nu(x_i) = q1px[0] n[e] + q1px[1] n[e + 1].
// With a = du_L, b = du_U, p = pn_L, q = pn_U the x-derivative at height c is (1 - c) a + c b and the x-summed nu (1 - c) p + c q, so
//     sum_g W nu u_x^2 = hs0^2 ( a^2 (p r30 + q r21) + 2 a b (p r21 + q r12) + b^2 (p r12 + q r03) ),
// and the y-derivative term is the same cubic in the per-node differences V[n] = u_U[n] - u_L[n] and the per-node y-moments S[n] of nu
// with the x-moments of the rule.  xm / ym carry hs^2 (ElemTab::q1xm / q1ym): e accumulates the element's  sum_g W nu |grad u|^2  as it
// is, and alpha enters where the cotangents are added to the nodes (an FMA in place of an add: alpha = 0, the energy of c = 0, costs nothing).
// ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ void q1cf_stage(const float px0, const float px1, const float u0, const float u1, const float n0, const float n1,
                                                    float& du, float& pn) {
    du = u1 - u0;
    pn = fmaf(px1, n1, px0 * n0);
}

__host__ __device__ __forceinline__ void q1cf_elem(const float (&xm)[4], const float (&ym)[4], const float a, const float b, const float p,
                                                   const float q, const float V0, const float V1, const float S0, const float S1,
                                                   const float alpha, float& gL0, float& gL1, float& gU0, float& gU1, float& e) {
    const float X0 = fmaf(q, xm[1], p * xm[0]), X1 = fmaf(q, xm[2], p * xm[1]), X2 = fmaf(q, xm[3], p * xm[2]);
    const float ta = fmaf(b, X1, a * X0), tb = fmaf(b, X2, a * X1);               // cotangents of du_L, du_U
    const float Y0 = fmaf(S1, ym[1], S0 * ym[0]), Y1 = fmaf(S1, ym[2], S0 * ym[1]), Y2 = fmaf(S1, ym[3], S0 * ym[2]);
    const float t0 = fmaf(V1, Y1, V0 * Y0), t1 = fmaf(V1, Y2, V0 * Y1);           // cotangents of V[e], V[e + 1]
    e = fmaf(b, tb, fmaf(a, ta, e));
    e = fmaf(V1, t1, fmaf(V0, t0, e));
    gL0 = fmaf(-alpha, ta + t0, gL0);
    gL1 = fmaf(alpha, ta - t1, gL1);
    gU0 = fmaf(alpha, t0 - tb, gU0);
    gU1 = fmaf(alpha, tb + t1, gU1);
}

// ---------------------------------------------------------------------------------------------
// 3-D Q1, marching form.  One element between node planes k (L) and k+1 (U), given each plane's in-plane stage at
// the element's in-plane Gauss points m = (jg, ig):
//   VU[jg][ig] value of u, VX[jg] = lerp_y of the x-differences, VY[ig] = y-difference of the x-lerped rows (all three as raw
//   differences: 1/h^2, alpha and the user scale are applied once per element, T.kap, T.hs2),
//   VNw = w_j w_i nu and VFw = w_j w_i f, the coefficient planes WEIGHTED (once per plane instead of once per layer, plane and term).
// As in 2-D every sum over the z-Gauss points collapses onto the moments of the 1-D rule, and the sums over one in-plane index
// onto small vectors (per jg and per ig): O(NGP^2) work per element.
// UW: all weights of the rule are 1 (the exact 2-point rule): weight multiplications vanish at compile time.
// Outputs: tU/tX/tY = complete cotangents of the LOWER plane's stage values (carry included), cU/cX/cY (in/out) = carried
// cotangents: in = from the layer below, out = this layer's contribution to the UPPER plane.  e1, e2 without wscale.
// ---------------------------------------------------------------------------------------------
template <int NGP, bool FGP, bool HAS_F, bool UW, typename V = float>
__device__ __forceinline__ void q1_layer_3d_w(const ElemTab& T, const V (&LU)[NGP][NGP], const V (&UU)[NGP][NGP],
                                              const V (&LX)[NGP], const V (&UX)[NGP], const V (&LY)[NGP],
                                              const V (&UY)[NGP], const V (&LN)[NGP][NGP], const V (&UN)[NGP][NGP],
                                              const V (&LF)[NGP][NGP], const V (&UF)[NGP][NGP],
                                              const float* fg, V (&cU)[NGP][NGP], V (&cX)[NGP], V (&cY)[NGP],
                                              V (&tU)[NGP][NGP], V (&tX)[NGP], V (&tY)[NGP], V& e1, V& e2) {
    V a1z = 0.f, a1x = 0.f, a1y = 0.f, a2 = 0.f;
    const float nb = T.nbw;
    // row / column sums of the weighted nu planes (x- and y-moments of nu at the y- / x-Gauss points)
    V LA[NGP], UA[NGP], LB[NGP], UB[NGP];
#pragma unroll
    for (int j = 0; j < NGP; ++j) {
        V la = 0.f, ua = 0.f, lb = 0.f, ub = 0.f;
#pragma unroll
        for (int i = 0; i < NGP; ++i) { la += LN[j][i]; ua += UN[j][i]; lb += LN[i][j]; ub += UN[i][j]; }
        LA[j] = la; UA[j] = ua; LB[j] = lb; UB[j] = ub;
    }
#pragma unroll
    for (int j = 0; j < NGP; ++j) {
#pragma unroll
        for (int i = 0; i < NGP; ++i) {
            const V dzu = UU[j][i] - LU[j][i];
            const V Qz = vfma(T.m[1], UN[j][i], T.m01 * LN[j][i]);          // sum_k w_k nu(i,j,k), in-plane weights inside
            const V qz = Qz * dzu;
            a1z = vfma(qz, dzu, a1z);
            V up = T.kap[2] * qz;                                            // cotangent of UU from the z-derivative term
            V lo = cU[j][i] - up;
            if constexpr (FGP) {
                V cs = 0.f, c1 = 0.f;
#pragma unroll
                for (int k = 0; k < NGP; ++k) {
                    const float wf = T.w[k] * T.w[j] * T.w[i] * fg[(k * NGP + j) * NGP + i];
                    cs += wf;
                    c1 = vfma(T.b[k][1], wf, c1);
                }
                a2 = vfma(cs, LU[j][i], a2);
                a2 = vfma(c1, dzu, a2);
                up = vfma(nb, c1, up);
                lo = vfma(nb, cs - c1, lo);
            } else if constexpr (HAS_F) {
                const V cs = vfma(T.m[1], UF[j][i], T.m01 * LF[j][i]);       // m0 FL + m1 (FU - FL)
                const V c1 = vfma(T.m[2], UF[j][i], T.m12 * LF[j][i]);       // m1 FL + m2 (FU - FL)
                a2 = vfma(cs, LU[j][i], a2);
                a2 = vfma(c1, dzu, a2);
                up = vfma(nb, c1, up);
                lo = vfma(nb, cs - c1, lo);
            }
            tU[j][i] = lo;
            cU[j][i] = up;
        }
    }
#pragma unroll
    for (int j = 0; j < NGP; ++j) {
        const V dX = UX[j] - LX[j], dA = UA[j] - LA[j];
        V sx = 0.f, tx = 0.f;
#pragma unroll
        for (int k = 0; k < NGP; ++k) {
            const V ux = vfma(T.b[k][1], dX, LX[j]);
            const V Qx = vfma(T.b[k][1], dA, LA[j]);
            const V qx = UW ? Qx * ux : (T.w[k] * Qx) * ux;
            a1x = vfma(qx, ux, a1x);
            sx += qx;
            tx = vfma(T.b[k][1], qx, tx);
        }
        const V up = T.kap[0] * tx;
        tX[j] = vfma(T.kap[0], sx, cX[j] - up);
        cX[j] = up;
    }
#pragma unroll
    for (int i = 0; i < NGP; ++i) {
        const V dY = UY[i] - LY[i], dB = UB[i] - LB[i];
        V sy = 0.f, ty = 0.f;
#pragma unroll
        for (int k = 0; k < NGP; ++k) {
            const V uy = vfma(T.b[k][1], dY, LY[i]);
            const V Qy = vfma(T.b[k][1], dB, LB[i]);
            const V qy = UW ? Qy * uy : (T.w[k] * Qy) * uy;
            a1y = vfma(qy, uy, a1y);
            sy += qy;
            ty = vfma(T.b[k][1], qy, ty);
        }
        const V up = T.kap[1] * ty;
        tY[i] = vfma(T.kap[1], sy, cY[i] - up);
        cY[i] = up;
    }
    e1 = vfma(T.hs2[2], a1z, vfma(T.hs2[0], a1x, T.hs2[1] * a1y));
    e2 = a2;
}

}  // namespace dn
