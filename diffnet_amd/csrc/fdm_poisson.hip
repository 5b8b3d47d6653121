// Fused 2-D finite-difference Poisson residual, its sums of squares and its gradient: dn_fdm_poisson_apply (include/diffnet_hip.h).
//
// The loss bodies of the three DiffNetFDM scripts of the reference under examples/poisson/single_instance/: 12_fdm_mms.py:76-118,
// 12_klsum_fdm.py:69-111 and 12_klsum_fdm_nbc.py:69-158 -- the two Dirichlet substitutions of u, six valid 3x3 conv2d calls (sobelx,
// sobely, sobelxx, sobelyy on u; sobelx, sobely on nu), the elementwise passes that form the residual, the sum of squares, the two
// Neumann row terms and, what autograd does for the scripts, the gradient with respect to u -- in ONE launch that reads u, nu and f once.
//
//   u~  = u after the two conditions (nu and f untouched);   kl = kxx + kyy;   (k * v)_i = sum_d k[d] v_{i+d}: the valid correlation
//   r_i = fs f_i + (kx * u~)_i (kx * nu)_i + (ky * u~)_i (ky * nu)_i + nu_i (kl * u~)_i            on the (ny-2) x (nx-2) interior
//   pullback:  d(sum r^2)/du~_j = 2 sum_d ( kx[d] a_{j-d} + ky[d] b_{j-d} + kl[d] c_{j-d} ),   a = r (kx * nu),  b = r (ky * nu),  c = r nu
//   (a, b, c zero outside the interior): three 3x3 adjoint stencils on three per-node products.
//
// Row march: one wave = FDM_OWNERS owner columns + two ghost lanes on either side (u is needed two columns beyond an owned node: one for
// the residual of the neighbour column, one more for that residual's own stencil); lane l holds node column chunk * FDM_OWNERS + l - 2.
// A lane marches the node rows of a strip; every row is loaded once, its x neighbours come from the neighbouring lanes (ds_bpermute),
// a row's three horizontal dot products per stencil are added into the rolling sums of the three residual rows it touches, and a
// finished residual row is scattered the same way into the rolling sums of the three gradient rows it touches.  A strip recomputes
// the seams: it loads two rows beyond either end and recomputes one residual row there.  Every output is written once, by its owner
// lane, from additions made in the same order in any strip: no atomics on the data path, res and grad bitwise independent of the launch
// plan and of the batch.  Sums: per thread in fp64 (the products r r are exact there), then the fixed-order fp64 reduction of
// dn_reduce.h, per sample.
//
// Optional inputs are compile-time forms: MASK (any condition), BCF (any value field), NU (nodal coefficient), FF (nodal forcing),
// GRAD (the gradient is wanted: without it the adjoint half is not compiled in).
#include <algorithm>
#include <cstdio>

#include "dn_reduce.h"

namespace dn {

constexpr int FDM_OWNERS = 60;             // owner lanes per wave (lanes 2 .. 61); lanes 0, 1, 62, 63 are ghosts that only supply the x halo
constexpr int FDM_MIN_ROWS = 16;           // shortest strip the library chooses: a strip loads four rows and recomputes two residual rows more

struct FdmParams {
    const float* u;
    const float* nu;                       // NU kernels
    const float* f;                        // FF kernels
    int nu_batched, f_batched;
    float nuv, fv, fs;                     // constant nu / f where the field is absent
    const void* mask[2];
    int mask_kind[2];                      // 0: none, 1: uint8 (!= 0), 2: fp32 (> 0.5)
    int mask_batched[2];
    const float* bcf[2];
    int bcf_batched[2];
    float bcv[2];
    float kx[9], ky[9], kl[9];             // row-major, x fastest; kl = kxx + kyy
    float gs_r, gs_n;                      // 2 out_scale | 2 out_scale nbc_scale
    const float* in_scale;                 // optional [B]
    float* res;
    float* grad;
    double* sums;                          // [B][3]
    double* part;                          // [3][nblocks]
    unsigned* counter;
    int nx, ny, chunks, rows_per_strip, strips, want_sums;
};

// Raw loads of node row t (clamped into the grid); the forcing is that of row t - 1, the residual row the landed row completes
template <bool MASK, bool BCF>
struct FdmRaw {
    float v, nu, f;
    float mf[MASK ? 2 : 1];
    uint8_t mb[MASK ? 2 : 1];
    float bf[BCF ? 2 : 1];
};

// k[m][0] l + k[m][1] c + k[m][2] r added to acc: row m of a correlation kernel on a node and its x neighbours
__device__ __forceinline__ float fdm_hrow(const float (&k)[9], int m, float l, float c, float r, float acc) {
    return fmaf(k[3 * m + 2], r, fmaf(k[3 * m + 1], c, fmaf(k[3 * m], l, acc)));
}
// ... of the adjoint: the node at x - 1 reaches x through k[m][2], the one at x + 1 through k[m][0]
__device__ __forceinline__ float fdm_hrow_t(const float (&k)[9], int m, float l, float c, float r, float acc) {
    return fmaf(k[3 * m], r, fmaf(k[3 * m + 1], c, fmaf(k[3 * m + 2], l, acc)));
}

// The per-sample final reduction: every workgroup leaves its three fp64 sums, the one that arrives last adds, for every sample, the
// partials of that sample's workgroups in index order (one wave per sum, lanes stride the partials, fixed shuffle tree) -- the same
// bits for a sample whatever the batch around it.
__device__ __forceinline__ void fdm_finish(const FdmParams& p, const double (&sq)[3], int tid, int nthreads, double* red, int* flag) {
    const int nblocks = launch_workgroups();
    double* parts[3];
    double mine[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        parts[k] = p.part + k * (size_t)nblocks;
        mine[k] = block_sum(sq[k], red, tid, nthreads);
    }
    if (tid == 0) {
        const int blk = workgroup_index();
        store_partials<3, true>(parts, blk, mine);
        *flag = arrive_last<false>(p.counter, nblocks, blk) ? 1 : 0;
    }
    __syncthreads();
    if (!*flag) return;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    const int gx = (int)gridDim.x, B = (int)gridDim.y;          // workgroup (x, b) has index b * gx + x
    const int wave = tid >> 6, lane = tid & 63, nw = nthreads >> 6;
    for (int pair = wave; pair < 3 * B; pair += nw) {
        const int b = pair / 3, k = pair - 3 * b;
        double acc = 0.0;
        for (int i = lane; i < gx; i += 64) acc += __hip_atomic_load(&parts[k][(size_t)b * gx + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        acc = wave_sum(acc);
        if (lane == 0) p.sums[pair] = acc;
    }
    if (tid == 0) {
        arrival_reset(p.counter);
        p.counter[DN_WS_TICKET_WORD] = 0u;
    }
}

template <bool MASK, bool BCF, bool NU, bool FF, bool GRAD>
__global__ void __launch_bounds__(256) fdm_poisson_kernel(const FdmParams p) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = (int)threadIdx.x & 63;
    const int wid = (int)blockIdx.x * ((int)blockDim.x >> 6) + wave;
    const int chunk = wid % p.chunks, strip = wid / p.chunks;      // strip >= p.strips: a wave of the last workgroup with nothing to do

    __shared__ double red[16];
    __shared__ int last_flag;
    double sq[3] = {0.0, 0.0, 0.0};                               // sum r^2 | Neumann row 0 | Neumann row ny - 1

    if (strip < p.strips) {
        const int nx = p.nx, ny = p.ny;
        const int q = chunk * FDM_OWNERS + lane - 2;
        const bool owner = lane >= 2 && lane < 2 + FDM_OWNERS && q < nx;
        const unsigned qc = (unsigned)min(max(q, 0), nx - 1);
        const bool col_in = q >= 1 && q <= nx - 2;
        const int b = blockIdx.y;
        const int64_t nps = (int64_t)nx * ny;

        const float* ub = p.u + (int64_t)b * nps;
        const float* nub = NU ? p.nu + (p.nu_batched ? (int64_t)b * nps : 0) : ub;
        const float* fb = FF ? p.f + (p.f_batched ? (int64_t)b * nps : 0) : ub;
        float* gb = GRAD ? p.grad + (int64_t)b * nps : nullptr;
        float* rb = p.res ? p.res + (int64_t)b * (nx - 2) * (ny - 2) : nullptr;
        const float* bcfb[2];
        const float* mfp[2];
        const uint8_t* mbp[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            bcfb[k] = p.bcf[k] ? p.bcf[k] + (p.bcf_batched[k] ? (int64_t)b * nps : 0) : ub;
            const int64_t mo = p.mask_batched[k] ? (int64_t)b * nps : 0;
            mfp[k] = reinterpret_cast<const float*>(p.mask[k]) + (p.mask_kind[k] == 2 ? mo : 0);
            mbp[k] = reinterpret_cast<const uint8_t*>(p.mask[k]) + (p.mask_kind[k] == 1 ? mo : 0);
        }
        float gs_r = p.gs_r;
        if constexpr (GRAD) {
            if (p.in_scale) gs_r *= p.in_scale[b];
        }

        using Raw = FdmRaw<MASK, BCF>;

        auto issue = [&](int t, Raw& w) {
            const unsigned rowoff = (unsigned)min(max(t, 0), ny - 1) * (unsigned)nx + qc;
            w.v = ld_at<float>(ub, rowoff);
            if constexpr (NU) w.nu = ld_at<float>(nub, rowoff);
            if constexpr (FF) w.f = ld_at<float>(fb, (unsigned)min(max(t - 1, 0), ny - 1) * (unsigned)nx + qc);
            if constexpr (MASK) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    w.mf[k] = 0.f;
                    w.mb[k] = 0;
                    if (p.mask_kind[k] == 2) w.mf[k] = ld_at<float>(mfp[k], rowoff);
                    else if (p.mask_kind[k] == 1) w.mb[k] = ld_at<uint8_t>(mbp[k], rowoff);
                }
            }
            if constexpr (BCF) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    w.bf[k] = 0.f;
                    if (p.bcf[k]) w.bf[k] = ld_at<float>(bcfb[k], rowoff);
                }
            }
        };

        const int j0 = strip * p.rows_per_strip, j1 = min(j0 + p.rows_per_strip, ny);

        // rolling sums of the residual rows in flight: X1 of row t - 1 (kernel rows 0, 1 added), X0 of row t (kernel row 0 added)
        float ux0 = 0.f, uy0 = 0.f, ul0 = 0.f, nx0 = 0.f, ny0 = 0.f;
        float ux1 = 0.f, uy1 = 0.f, ul1 = 0.f, nx1 = 0.f, ny1 = 0.f;
        // ... of the gradient rows: g1 of row t - 2, g0 of row t - 1
        float g0 = 0.f, g1 = 0.f;
        float nu_prev = 0.f;                                      // nu of row t - 1
        float u1 = 0.f, u2 = 0.f, u3 = 0.f;                       // u~ of rows t - 1, t - 2, t - 3 (the Neumann terms of row t - 2)
        unsigned fixed_bits = 0u;                                 // bit i: row t - i is a Dirichlet node

        // node row t has landed in W: finishes residual row t - 1 and gradient row t - 2; W is refilled with row t + 2
        auto step = [&](int t, Raw& W) {
            float uc = W.v, nuc = p.nuv, fc = p.fv;
            if constexpr (NU) nuc = W.nu;
            if constexpr (FF) fc = W.f;
            bool fixed = false;
            if constexpr (MASK) {
                bool fx[2];
                float bv[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    fx[k] = p.mask_kind[k] == 2 ? (W.mf[k] > 0.5f) : (p.mask_kind[k] == 1 ? (W.mb[k] != 0) : false);
                    bv[k] = p.bcv[k];
                    if constexpr (BCF) bv[k] = p.bcf[k] ? W.bf[k] : bv[k];
                }
                fixed = fx[0] || fx[1];
                uc = fx[1] ? bv[1] : (fx[0] ? bv[0] : uc);        // applied in order: condition 2 wins
            }
            issue(t + 2, W);
            fixed_bits = (fixed_bits << 1) | (fixed ? 1u : 0u);

            const float ul = __shfl_up(uc, 1, 64), ur = __shfl_down(uc, 1, 64);
            float nl = nuc, nr = nuc;
            if constexpr (NU) {
                nl = __shfl_up(nuc, 1, 64);
                nr = __shfl_down(nuc, 1, 64);
            }
            // residual row s = t - 1: kernel row 2 closes it
            const int s = t - 1;
            const float dux = fdm_hrow(p.kx, 2, ul, uc, ur, ux1), duy = fdm_hrow(p.ky, 2, ul, uc, ur, uy1);
            const float lap = fdm_hrow(p.kl, 2, ul, uc, ur, ul1);
            const float dnx = fdm_hrow(p.kx, 2, nl, nuc, nr, nx1), dny = fdm_hrow(p.ky, 2, nl, nuc, nr, ny1);
            ux1 = fdm_hrow(p.kx, 1, ul, uc, ur, ux0); uy1 = fdm_hrow(p.ky, 1, ul, uc, ur, uy0);
            ul1 = fdm_hrow(p.kl, 1, ul, uc, ur, ul0);
            nx1 = fdm_hrow(p.kx, 1, nl, nuc, nr, nx0); ny1 = fdm_hrow(p.ky, 1, nl, nuc, nr, ny0);
            ux0 = fdm_hrow(p.kx, 0, ul, uc, ur, 0.f); uy0 = fdm_hrow(p.ky, 0, ul, uc, ur, 0.f);
            ul0 = fdm_hrow(p.kl, 0, ul, uc, ur, 0.f);
            nx0 = fdm_hrow(p.kx, 0, nl, nuc, nr, 0.f); ny0 = fdm_hrow(p.ky, 0, nl, nuc, nr, 0.f);

            const bool inside = col_in && s >= 1 && s <= ny - 2;
            float r = fmaf(nu_prev, lap, fmaf(duy, dny, fmaf(dux, dnx, p.fs * fc)));
            r = inside ? r : 0.f;
            const bool mine = owner && s >= j0 && s < j1;
            if (mine) {
                sq[0] = fma((double)r, (double)r, sq[0]);
                if (rb && inside) st_at<float>(rb, (unsigned)(s - 1) * (unsigned)(nx - 2) + (unsigned)(q - 1), r);
            }

            const int j = t - 2;
            const bool out_row = j >= j0 && j < j1;               // wave-uniform
            if constexpr (GRAD) {
                const float a = r * dnx, bb = r * dny, c = r * nu_prev;
                const float al = __shfl_up(a, 1, 64), ar = __shfl_down(a, 1, 64);
                const float bl = __shfl_up(bb, 1, 64), br = __shfl_down(bb, 1, 64);
                const float cl = __shfl_up(c, 1, 64), cr = __shfl_down(c, 1, 64);
                // gradient row j = s - 1: kernel row 0 of the products of row s closes it
                const float g = fdm_hrow_t(p.kl, 0, cl, c, cr, fdm_hrow_t(p.ky, 0, bl, bb, br, fdm_hrow_t(p.kx, 0, al, a, ar, g1)));
                g1 = fdm_hrow_t(p.kl, 1, cl, c, cr, fdm_hrow_t(p.ky, 1, bl, bb, br, fdm_hrow_t(p.kx, 1, al, a, ar, g0)));
                g0 = fdm_hrow_t(p.kl, 2, cl, c, cr, fdm_hrow_t(p.ky, 2, bl, bb, br, fdm_hrow_t(p.kx, 2, al, a, ar, 0.f)));
                if (out_row) {
                    // d/du~ of (u~[0] - u~[1])^2 and (u~[ny-1] - u~[ny-2])^2 without the factor 2 (gs_n carries it); ny == 3: row 1 takes both
                    float nb = 0.f;
                    nb = j == 0 ? u2 - u1 : nb;
                    nb = j == 1 ? nb - (u3 - u2) : nb;
                    nb = j == ny - 2 ? nb - (u1 - u2) : nb;
                    nb = j == ny - 1 ? nb + (u2 - u3) : nb;
                    float val = fmaf(p.gs_n, nb, gs_r * g);
                    if constexpr (MASK) val = (fixed_bits & 4u) ? 0.f : val;     // no gradient reaches a substituted node
                    if (owner) st_at<float>(gb, (unsigned)j * (unsigned)nx + qc, val);
                }
            }
            if (out_row && owner && (j == 0 || j == ny - 1)) {
                const double d0 = (double)u2 - (double)u1, d1 = (double)u2 - (double)u3;
                if (j == 0) sq[1] = fma(d0, d0, sq[1]);
                if (j == ny - 1) sq[2] = fma(d1, d1, sq[2]);
            }
            nu_prev = nuc;
            u3 = u2; u2 = u1; u1 = uc;
        };

        // two rows in flight ahead of the one being consumed (W0, W1 alternate; unrolled by two so that no register with a load
        // outstanding is ever copied)
        Raw W0, W1;
        issue(j0 - 2, W0);
        issue(j0 - 1, W1);
        for (int t = j0 - 2; t <= j1 + 1; t += 2) {
            step(t, W0);
            if (t + 1 <= j1 + 1) step(t + 1, W1);
        }
    }
    if (p.want_sums) fdm_finish(p, sq, (int)threadIdx.x, (int)blockDim.x, red, &last_flag);
}

#define FDM_LAUNCH(...) hipLaunchKernelGGL((fdm_poisson_kernel<__VA_ARGS__>), grid, block, 0, s, pp)

// MASK / BCF: sel 0 none, 1 conditions with constants, 2 with a value field
template <bool NU, bool FF, bool GRAD>
static void fdm_launch_mask(const FdmParams& pp, int sel, dim3 grid, dim3 block, hipStream_t s) {
    if (sel == 2) FDM_LAUNCH(true, true, NU, FF, GRAD);
    else if (sel == 1) FDM_LAUNCH(true, false, NU, FF, GRAD);
    else FDM_LAUNCH(false, false, NU, FF, GRAD);
}

template <bool NU, bool FF>
static void fdm_launch_grad(const FdmParams& pp, int sel, dim3 grid, dim3 block, hipStream_t s) {
    if (pp.grad) fdm_launch_mask<NU, FF, true>(pp, sel, grid, block, s);
    else fdm_launch_mask<NU, FF, false>(pp, sel, grid, block, s);
}

struct FdmGeom { int chunks, strips, R, wpb, gx; };

static inline int fdm_validate(int B, int ny, int nx) {
    if (B < 1 || B > 65535 || ny < 3 || nx < 3) return DN_E_BADARG;
    if ((int64_t)nx * ny >= (1ll << 30)) return DN_E_UNSUPPORTED;           // 32-bit byte offsets within a sample
    return 0;
}

// One wave per (60-column chunk, strip of R node rows, sample), four waves per workgroup; strips as short as FDM_MIN_ROWS until the
// launch has ~4096 waves (16 per CU: the rows stream from HBM, their latency is hidden by the other waves of the SIMD and the
// prefetch).  "PLAN_FSDT" ("T,R": T = 64 x waves per workgroup, R node rows per strip) overrides both, as it does for the element
// forms; res and grad do not depend on the plan.
static inline FdmGeom fdm_plan(int B, int ny, int nx) {
    FdmGeom g;
    g.chunks = (nx + FDM_OWNERS - 1) / FDM_OWNERS;
    const int64_t per_row = (int64_t)g.chunks * B;
    int strips = (int)std::min<int64_t>((4096 + per_row - 1) / per_row, (ny + FDM_MIN_ROWS - 1) / FDM_MIN_ROWS);
    strips = std::max(strips, 1);
    int R = (ny + strips - 1) / strips, wpb = 4;
    const char* e = config(CFG_PLAN_FSDT);
    int T, RR;
    if (e && sscanf(e, "%d,%d", &T, &RR) == 2 && T >= 64 && T <= 256 && T % 64 == 0 && RR >= 1) {
        wpb = T / 64;
        R = RR;
    }
    g.R = std::max(1, std::min(R, ny));
    g.strips = (ny + g.R - 1) / g.R;
    const int waves = g.chunks * g.strips;
    g.wpb = std::min(waves, wpb);
    g.gx = (waves + g.wpb - 1) / g.wpb;
    return g;
}

// three partial sums per workgroup, for an upper bound of the workgroups over every launch plan (one-wave workgroups, one-row strips):
// the size does not change with "PLAN_FSDT"
static inline int64_t fdm_workspace_bytes(int B, int ny, int nx) {
    const int64_t chunks = (nx + FDM_OWNERS - 1) / FDM_OWNERS;
    return DN_WS_HEADER + (int64_t)(3 * sizeof(double)) * chunks * ny * B;
}

}  // namespace dn

using namespace dn;

extern "C" int64_t dn_fdm_poisson_workspace_bytes(int32_t B, int32_t ny, int32_t nx) {
    if (fdm_validate(B, ny, nx) != 0) return DN_E_BADARG;
    return fdm_workspace_bytes(B, ny, nx);
}

extern "C" int dn_fdm_poisson_apply(const dn_fdm_poisson_args* a, void* stream) {
    if (!a) return DN_E_BADARG;
    const int B = a->B, ny = a->ny, nx = a->nx;
    int rc = fdm_validate(B, ny, nx);
    if (rc) return rc;
    if (!a->u) return DN_E_BADARG;
    if (!a->res && !a->sums && !a->grad) return DN_E_BADARG;
    if ((a->nu_batched | a->f_batched) & ~1) return DN_E_BADARG;
    for (int k = 0; k < 2; ++k) {
        const dn_dirichlet& d = a->bc[k];
        if (d.mask_kind == DN_MASK_BITS || d.mask_kind == DN_MASK_BOX) return DN_E_UNSUPPORTED;     // expand them: dn_unpack_mask_bits
        if (d.mask_kind != DN_MASK_F32 && d.mask_kind != DN_MASK_U8) return DN_E_BADARG;
        if ((d.mask_batched | d.field_batched) & ~1) return DN_E_BADARG;
        if (d.field && !d.mask) return DN_E_BADARG;                           // a value field without its mask
    }
    if (a->sums && (!a->workspace || a->workspace_bytes < fdm_workspace_bytes(B, ny, nx))) return DN_E_WORKSPACE;
    const FdmGeom g = fdm_plan(B, ny, nx);

    FdmParams pp;
    pp.u = a->u;
    pp.nu = a->nu;
    pp.f = a->f;
    pp.nu_batched = a->nu_batched;
    pp.f_batched = a->f_batched;
    pp.nuv = a->nu ? 0.f : a->nu_value;
    pp.fv = a->f ? 0.f : a->f_value;
    pp.fs = a->fs;
    bool mask = false, bcf = false;
    for (int k = 0; k < 2; ++k) {
        const dn_dirichlet& d = a->bc[k];
        pp.mask[k] = d.mask;
        pp.mask_kind[k] = !d.mask ? 0 : (d.mask_kind == DN_MASK_U8 ? 1 : 2);
        pp.mask_batched[k] = d.mask_batched;
        pp.bcf[k] = d.field;
        pp.bcf_batched[k] = d.field_batched;
        pp.bcv[k] = d.value;
        mask = mask || d.mask;
        bcf = bcf || d.field;
    }
    for (int i = 0; i < 9; ++i) {
        pp.kx[i] = a->kx[i];
        pp.ky[i] = a->ky[i];
        pp.kl[i] = a->kxx[i] + a->kyy[i];
    }
    pp.gs_r = 2.f * a->out_scale;
    pp.gs_n = 2.f * a->out_scale * a->nbc_scale;
    pp.in_scale = a->in_scale;
    pp.res = a->res;
    pp.grad = a->grad;
    pp.sums = a->sums;
    pp.counter = reinterpret_cast<unsigned*>(a->workspace);
    pp.part = a->workspace ? reinterpret_cast<double*>(reinterpret_cast<char*>(a->workspace) + DN_WS_HEADER) : nullptr;
    pp.nx = nx; pp.ny = ny;
    pp.chunks = g.chunks; pp.rows_per_strip = g.R; pp.strips = g.strips;
    pp.want_sums = a->sums ? 1 : 0;

    const dim3 grid(g.gx, B), block(64 * g.wpb);
    const int sel = mask ? (bcf ? 2 : 1) : 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (pp.nu) {
        if (pp.f) fdm_launch_grad<true, true>(pp, sel, grid, block, s);
        else fdm_launch_grad<true, false>(pp, sel, grid, block, s);
    } else {
        if (pp.f) fdm_launch_grad<false, true>(pp, sel, grid, block, s);
        else fdm_launch_grad<false, false>(pp, sel, grid, block, s);
    }
    DN_LAUNCH_CHECK();
    return 0;
}
