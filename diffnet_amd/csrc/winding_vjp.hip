// Vector-Jacobian product of the general winding-number field (winding_field.hip) with respect to the cloud: for
//   w[b, q] = scale * sum_p a_p (d . n_p) inv(d),   d = x_p - q,   a_p = 1 without area
// and a cotangent g[b, q], with num = d . n_p:
//   L2:  inv = r^-power,  r = |d|_2,      dinv_i = -power d_i r^-(power + 2)
//   L1:  inv = s^-power,  s = sum |d_i|,  dinv_i = -power sgn(d_i) s^-(power + 1),   sgn(0) = 0 (torch's convention)
//   grad_area[b, p]       = scale       sum_q g num inv
//   grad_normals[b, p, i] = scale a_p   sum_q g d_i inv
//   grad_points[b, p, i]  = scale a_p   sum_q g (n_i inv + num dinv_i)
// It differentiates the same reference forms as the forward (compute_winding_torch,
// examples/eiqonal/single_instance/02_differentiable_winding_number.py:15-30, and the 2-D compute_winding_gpts / compute_winding_nodes).
// Queries are constants here.
//
// Tiling: the forward's, with the roles of points and queries swapped.  A workgroup of 256 threads owns 256 consecutive points of one
// sample; a thread keeps x, n and the 1 + 2 dim accumulators of its point in registers.  The queries pass through LDS in chunks of 256,
// staged together with their cotangent as (q_x, q_y, q_z, g) -- 2-D: (q_x, q_y, g) in a 16-byte slot --, one broadcast ds_read_b128 per
// pair.  g belongs to the sample, so the sample is a grid dimension.  A cloud is small and a mesh large, so the query range is split
// over S slices of whole chunks, grid (ceil(npts / 256), S, B); slice s takes chunks [s C / S, (s + 1) C / S) of the C = ceil(nq / 256).
// The 1 + 2 dim fp32 accumulators of a thread are G = sum g inv, N_i = sum g d_i inv and C_i = sum g num dinv_i; n_p is the thread's
// own, so the sums of the formulas are n . N (area), N_i (normals) and n_i G + C_i (points), formed in float64 at the end of a chunk.
// Per pair, in VALU instructions (3-D L2 cubed): 3 sub, 1 mul + 2 fma (num), 1 mul + 2 fma (r^2), rsq, 3 mul (rs^2, inv, g inv),
// 2 mul (the common factor cf of num g dinv_i = cf d_i), 1 add + 3 fma + 3 fma = 21 + rsq against the forward's 12 + rsq (the
// compiled loop has 23 + rsq; the 3-D L1 cubed form 27 + rcp, 6 of them the three sgn(d_i)).
// The a_p of the formulas multiplies the finished sum, not each pair.
//
// Precision and order.  Inside one chunk every accumulator is one fp32 chain (fma; add for G and the L1 C_i) from zero in query order; at the
// end of the chunk it enters a float64 running sum (a handful of fp64 operations per 256 pairs).  With S == 1 the kernel finishes by itself; else a slice stores
// its float64 sums to the workspace [S][B][npts][1 + 2 dim] and winding_vjp_finish adds the slices in index order 0 .. S - 1.  Either
// way the sum is multiplied by scale (and a_p) in float64 and rounded once to float32, and every requested output is written once.  No
// atomics: the bits are repeatable for a given S and do not depend on which outputs are requested (launch-uniform branches around the
// stores only).  Across different S the float64 partial sums are cut at other chunks and the bits may differ in the last place -- weaker
// than the forward, whose bits do not depend on its tile at all.
//
// A packed-fp32 form with two points per thread (as the forward's Q >= 2) is not built: see profiles/winding_vjp.txt.
// A point that coincides with a query gives inf / nan as in the forward; nothing is clamped.
#include "dn_common.h"

namespace dn {

constexpr int WV_THREADS = 256;      // threads per workgroup = points per workgroup
constexpr int WV_CHUNK = 256;        // queries staged per pass
constexpr int WV_MAX_SLICES = 1024;
constexpr int64_t WV_TARGET_THREADS = (int64_t)64 * 256 * 256;         // 64 workgroups of 256 threads on each of 256 CUs

// sgn(d) = -1, 0 or 1, exactly, with sgn(0) = 0 (not a copysign): d 2^255 is 0, or at least 2^106 in size (inf for every normal d, and
// the smallest denormal is 2^-149), and the median with -1 and 1 cuts it to +-1.  Two instructions (v_ldexp_f32, v_med3_f32) where
// two compares and two selects take four.
__device__ __forceinline__ float wv_sgn(float d) { return __builtin_amdgcn_fmed3f(ldexpf(d, 255), -1.f, 1.f); }

// scale (and the point's area) onto the float64 sums, one rounding to float32, each requested output once
template <int DIM>
__device__ __forceinline__ void wv_store(const double (&sum)[1 + 2 * DIM], size_t p, const float* __restrict__ area, float scale,
                                         float* __restrict__ gp, float* __restrict__ gn, float* __restrict__ ga) {
    const double s = (double)scale;
    const double sa = area ? s * (double)area[p] : s;
    if (ga) ga[p] = (float)(s * sum[0]);
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
        if (gn) gn[p * DIM + i] = (float)(sa * sum[1 + i]);
        if (gp) gp[p * DIM + i] = (float)(sa * sum[1 + DIM + i]);
    }
}

// pts, nrm: (B, npts, DIM); area: (B, npts) or null; queries: (DIM, nq); g: (B, nq); ws: [S][B][npts][1 + 2 DIM] float64, or null when
// gridDim.y == 1 (the kernel then finishes: gp, gn (B, npts, DIM), ga (B, npts), each may be null)
template <int DIM, int METRIC, int POWER>
__global__ void __launch_bounds__(WV_THREADS) winding_vjp_kernel(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                                 const float* __restrict__ area, const float* __restrict__ queries,
                                                                 const float* __restrict__ g, double* __restrict__ ws,
                                                                 float* __restrict__ gp, float* __restrict__ gn, float* __restrict__ ga,
                                                                 int npts, int64_t nq, float scale) {
    constexpr int NA = 1 + 2 * DIM;
    __shared__ float4 sq[WV_CHUNK];                     // 3-D: (qx, qy, qz, g);  2-D: (qx, qy, g, -)
    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int p_own = blockIdx.x * WV_THREADS + tid;
    const bool live = p_own < npts;
    const size_t p = (size_t)b * (size_t)npts + (size_t)(live ? p_own : npts - 1);     // past the end: a copy of the last point, never stored
    float x[DIM], n[DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
        x[i] = pts[p * DIM + i];
        n[i] = nrm[p * DIM + i];
    }
    double sum[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) sum[k] = 0.0;
    const int64_t chunks = (nq + WV_CHUNK - 1) / WV_CHUNK;
    const int64_t c0 = chunks * (int64_t)blockIdx.y / (int64_t)gridDim.y, c1 = chunks * ((int64_t)blockIdx.y + 1) / (int64_t)gridDim.y;
    const float* __restrict__ gb = g + (size_t)b * (size_t)nq;
    for (int64_t c = c0; c < c1; ++c) {
        const int64_t qbase = c * WV_CHUNK;
        const int cnt = (int)min((int64_t)WV_CHUNK, nq - qbase);
        if (tid < cnt) {
            const int64_t q = qbase + tid;
            if constexpr (DIM == 2) sq[tid] = make_float4(queries[q], queries[nq + q], gb[q], 0.f);
            else sq[tid] = make_float4(queries[q], queries[nq + q], queries[2 * nq + q], gb[q]);
        }
        __syncthreads();
        float acc[NA];
#pragma unroll
        for (int k = 0; k < NA; ++k) acc[k] = 0.f;
#pragma unroll 2
        for (int j = 0; j < cnt; ++j) {
            const float4 v = sq[j];
            float d[DIM];
            d[0] = x[0] - v.x;
            d[1] = x[1] - v.y;
            if constexpr (DIM == 3) d[2] = x[2] - v.z;
            const float gq = DIM == 3 ? v.w : v.z;
            float num = d[0] * n[0];
#pragma unroll
            for (int i = 1; i < DIM; ++i) num = fmaf(d[i], n[i], num);
            float gi, cf;               // gi = g inv;  cf: num g dinv_i = cf d_i (L2) or cf sgn(d_i) (L1)
            if constexpr (METRIC == 0) {
                float s = fabsf(d[0]) + fabsf(d[1]);
                if constexpr (DIM == 3) s += fabsf(d[2]);
                const float r = __builtin_amdgcn_rcpf(s);
                float inv = r * r;
                if constexpr (POWER == 3) inv *= r;
                gi = gq * inv;
                cf = (num * gi) * (r * (float)-POWER);
            } else {
                float r2 = d[0] * d[0];
#pragma unroll
                for (int i = 1; i < DIM; ++i) r2 = fmaf(d[i], d[i], r2);
                const float rs = __builtin_amdgcn_rsqf(r2);
                const float rs2 = rs * rs;
                float inv = rs2;
                if constexpr (POWER == 3) inv *= rs;
                gi = gq * inv;
                cf = (num * gi) * (rs2 * (float)-POWER);
            }
            acc[0] += gi;
#pragma unroll
            for (int i = 0; i < DIM; ++i) {
                acc[1 + i] = fmaf(d[i], gi, acc[1 + i]);
                if constexpr (METRIC == 0) acc[1 + DIM + i] = fmaf(wv_sgn(d[i]), cf, acc[1 + DIM + i]);
                else acc[1 + DIM + i] = fmaf(d[i], cf, acc[1 + DIM + i]);
            }
        }
        // n is the thread's own: sum_q g num inv = n . sum_q g d inv, and sum_q g n_i inv = n_i sum_q g inv, exact products in float64
        double dot = 0.0;
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
            dot += (double)n[i] * (double)acc[1 + i];
            sum[1 + i] += (double)acc[1 + i];
            sum[1 + DIM + i] += (double)n[i] * (double)acc[0] + (double)acc[1 + DIM + i];
        }
        sum[0] += dot;
        __syncthreads();
    }
    if (!live) return;
    if (ws) {
        double* __restrict__ o = ws + (((size_t)blockIdx.y * gridDim.z + (size_t)b) * (size_t)npts + (size_t)p_own) * NA;
#pragma unroll
        for (int k = 0; k < NA; ++k) o[k] = sum[k];
    } else {
        wv_store<DIM>(sum, p, area, scale, gp, gn, ga);
    }
}

// one thread per point: the slices' float64 sums in index order, then wv_store
template <int DIM>
__global__ void __launch_bounds__(WV_THREADS) winding_vjp_finish(const double* __restrict__ ws, const float* __restrict__ area,
                                                                 float* __restrict__ gp, float* __restrict__ gn, float* __restrict__ ga,
                                                                 int npts, int slices, float scale) {
    constexpr int NA = 1 + 2 * DIM;
    const int p_own = blockIdx.x * WV_THREADS + threadIdx.x;
    if (p_own >= npts) return;
    const size_t p = (size_t)blockIdx.y * (size_t)npts + (size_t)p_own;
    const size_t stride = (size_t)gridDim.y * (size_t)npts * NA;
    double sum[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) sum[k] = 0.0;
    for (int s = 0; s < slices; ++s) {
#pragma unroll
        for (int k = 0; k < NA; ++k) sum[k] += ws[(size_t)s * stride + p * NA + k];
    }
    wv_store<DIM>(sum, p, area, scale, gp, gn, ga);
}

using WvKernel = void (*)(const float*, const float*, const float*, const float*, const float*, double*, float*, float*, float*, int,
                          int64_t, float);

static WvKernel wv_pick(int dim, int metric, int power) {
    const int key = (dim - 2) * 4 + metric * 2 + (power - 2);
    switch (key) {
        case 0: return winding_vjp_kernel<2, 0, 2>;
        case 1: return winding_vjp_kernel<2, 0, 3>;
        case 2: return winding_vjp_kernel<2, 1, 2>;
        case 3: return winding_vjp_kernel<2, 1, 3>;
        case 4: return winding_vjp_kernel<3, 0, 2>;
        case 5: return winding_vjp_kernel<3, 0, 3>;
        case 6: return winding_vjp_kernel<3, 1, 2>;
        default: return winding_vjp_kernel<3, 1, 3>;
    }
}

}  // namespace dn

// Slices of the query range for a problem: enough for 64 workgroups per CU (256 CUs), i.e. batch * npts * S >= 2^22 point threads,
// never more than the chunks of 256 queries there are and never more than 1024.  A CU holds 8 of these workgroups at a time (one wave
// each on its 4 SIMDs, 8 waves per SIMD), all workgroups of a launch take the same time, and what a launch loses is the last, partly
// filled round.  The first guess, four waves per SIMD as dn_winding_field_tile reasons, was too few: at 128^3 nodes x 10 242 points
// (41 workgroups per slice) its 26 slices -- 4.2 workgroups per CU -- took 15.5 ms, 64 slices 12.9, 256 slices 11.5 and 1024 slices
// 11.7; at 25^3 probes 16 / 26 / 62 slices (62 chunks) took 159 / 144 / 136 us (profiles/winding_vjp.txt).  The finishing pass reads
// 56 bytes per point and slice and does not show.
extern "C" int dn_winding_field_vjp_slices(int32_t batch, int32_t npts, int64_t nq) {
    if (batch < 1 || npts < 1 || nq < 1) return DN_E_BADARG;
    const int64_t threads = (int64_t)batch * npts;
    const int64_t chunks = (nq + dn::WV_CHUNK - 1) / dn::WV_CHUNK;
    int64_t s = (dn::WV_TARGET_THREADS + threads - 1) / threads;
    if (s > chunks) s = chunks;
    if (s > dn::WV_MAX_SLICES) s = dn::WV_MAX_SLICES;
    return (int)s;
}

extern "C" int64_t dn_winding_field_vjp_workspace_bytes(int32_t batch, int32_t npts, int32_t dim, int32_t slices) {
    if (batch < 1 || batch > 65535 || npts < 1 || (dim != 2 && dim != 3) || slices < 1 || slices > dn::WV_MAX_SLICES) return DN_E_BADARG;
    return (int64_t)slices * batch * npts * (1 + 2 * dim) * (int64_t)sizeof(double);       // < 2^63 for every valid argument
}

extern "C" int dn_winding_field_vjp(const float* points, const float* normals, const float* area, const float* queries,
                                    const float* grad_field, float* grad_points, float* grad_normals, float* grad_area, void* workspace,
                                    int64_t workspace_bytes, int32_t batch, int32_t npts, int64_t nq, int32_t dim, int32_t metric,
                                    int32_t power, float scale, int32_t slices, void* stream) {
    if (!points || !normals || !queries || !grad_field) return DN_E_BADARG;
    if (!grad_points && !grad_normals && !grad_area) return DN_E_BADARG;
    if (grad_area && !area) return DN_E_BADARG;
    if (dim != 2 && dim != 3) return DN_E_BADARG;
    if (power != 2 && power != 3) return DN_E_BADARG;
    if (metric != 0 && metric != 1) return DN_E_BADARG;
    if (batch < 1 || batch > 65535 || npts < 1 || nq < 1) return DN_E_BADARG;
    if (slices < 0 || slices > dn::WV_MAX_SLICES) return DN_E_BADARG;
    const int64_t chunks = (nq + dn::WV_CHUNK - 1) / dn::WV_CHUNK;
    int64_t s = slices ? slices : dn_winding_field_vjp_slices(batch, npts, nq);
    if (s > chunks) s = chunks;                         // no slice without a chunk
    if (s > 1 && (!workspace || workspace_bytes < dn_winding_field_vjp_workspace_bytes(batch, npts, dim, (int32_t)s))) return DN_E_WORKSPACE;
    const unsigned blocks = (unsigned)(((int64_t)npts + dn::WV_THREADS - 1) / dn::WV_THREADS);
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* ws = s > 1 ? static_cast<double*>(workspace) : nullptr;
    hipLaunchKernelGGL(dn::wv_pick(dim, metric, power), dim3(blocks, (unsigned)s, (unsigned)batch), dim3(dn::WV_THREADS), 0, st, points,
                       normals, area, queries, grad_field, ws, grad_points, grad_normals, grad_area, (int)npts, nq, scale);
    DN_LAUNCH_CHECK();
    if (s > 1) {
        if (dim == 2)
            hipLaunchKernelGGL(dn::winding_vjp_finish<2>, dim3(blocks, (unsigned)batch), dim3(dn::WV_THREADS), 0, st, ws, area, grad_points,
                               grad_normals, grad_area, (int)npts, (int)s, scale);
        else
            hipLaunchKernelGGL(dn::winding_vjp_finish<3>, dim3(blocks, (unsigned)batch), dim3(dn::WV_THREADS), 0, st, ws, area, grad_points,
                               grad_normals, grad_area, (int)npts, (int)s, scale);
        DN_LAUNCH_CHECK();
    }
    return 0;
}
