// General winding-number field of a point cloud with normals and area weights, 2-D or 3-D, on a flat list of queries:
//   w[b, q] = scale * sum_p area[b,p] * ((x_p - q) . n_p) / dist(x_p - q)^power
// dist = L1 norm (the quirk of the reference's compute_winding_* functions) or the Euclidean norm (the true generalised winding
// number with power = dim and scale = 1 / (2 pi), 1 / (4 pi)).  Reference forms this covers: compute_winding_torch
// (examples/eiqonal/single_instance/02_differentiable_winding_number.py:15-30: 3-D, L1, cubed, area), compute_winding_gpts
// (examples/poisson/single_instance/winding_immersed_background_2d.py:59-80: 2-D, L1, squared, area) and compute_winding_nodes (2-D, L1,
// cubed, no area, (4 pi)^-3 in front).
//
// Tiling.  A workgroup of 256 threads owns W = 256 Q consecutive queries, Q = 1, 2 or 4 per thread in registers (thread t holds queries
// t, t + 256, ...: loads and stores stay coalesced).  The cloud passes through LDS in chunks of C = 256 points, staged as
// (x, n * area): the area multiply is paid once per point and workgroup, not once per pair.  One point is one broadcast ds_read_b128
// (+ one ds_read_b64 in 3-D) per lane and serves all Q queries, where the one-query-per-thread kernel of winding.hip issues one LDS
// read per pair.  At Q >= 2 the queries of a thread are held two to a register pair and the loop body is packed fp32
// (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32: two queries per instruction, the point's value selected for both halves by op_sel);
// only |d_0| + |d_1| (+ |d_2|) stays one instruction per query, because the packed forms have no |.| source modifier, and the
// transcendental has no packed form.  Per pair of one point and one query, in VALU instructions (v_rcp_f32 / v_rsq_f32 issue at
// half the rate of the others):
//                    Q = 1                                                           Q >= 2 (per two queries)
//   3-D L1 cubed:    3 sub, 2 add, 2 mul, rcp, 1 mul + 2 fma, 1 fma      = 11 + rcp      3 + 4 + 2 + 3 + 1 = 13, + 2 rcp
//   2-D L1 cubed:    2 sub, 1 add, 2 mul, rcp, 1 mul + 1 fma, 1 fma      =  8 + rcp      2 + 2 + 2 + 2 + 1 =  9, + 2 rcp
//   3-D L2 cubed:    3 sub, 1 mul + 2 fma, rsq, 2 mul, 1 mul + 2 fma, 1 fma = 12 + rsq   3 + 3 + 2 + 3 + 1 = 12, + 2 rsq
// The accumulation chains of a thread are independent, which also hides the latency of the transcendental.
//
// Order.  Every query sums its points in index order 0 .. npts - 1 in one fma chain, and a packed instruction rounds each half as
// the plain one does: results are bitwise the same for every Q and grid.  No atomics, no split of the point loop over workgroups
// (DESIGN.md 3.2 has the measured cost of that at 25^3 probes).
//
// A point that coincides with a query gives inf / nan as in the reference; nothing is clamped.
#include <type_traits>
#include "dn_common.h"

namespace dn {

constexpr int WF_THREADS = 256;      // threads per workgroup
constexpr int WF_CHUNK = 256;        // points staged per pass (one per thread)
constexpr int64_t WF_MAX_BLOCKS = 0xFFFFFF;       // grid.x * 256 threads stays below 2^32

typedef float wf_f2 __attribute__((ext_vector_type(2)));

// one value per query (float) or two (wf_f2): the few operations the loop body needs beyond + - *
__device__ __forceinline__ float wf_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ wf_f2 wf_fma(wf_f2 a, wf_f2 b, wf_f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float wf_rcp(float a) { return __builtin_amdgcn_rcpf(a); }
__device__ __forceinline__ wf_f2 wf_rcp(wf_f2 a) { return wf_f2{__builtin_amdgcn_rcpf(a.x), __builtin_amdgcn_rcpf(a.y)}; }
__device__ __forceinline__ float wf_rsq(float a) { return __builtin_amdgcn_rsqf(a); }
__device__ __forceinline__ wf_f2 wf_rsq(wf_f2 a) { return wf_f2{__builtin_amdgcn_rsqf(a.x), __builtin_amdgcn_rsqf(a.y)}; }
template <int DIM>
__device__ __forceinline__ float wf_l1(const float (&d)[DIM]) {
    float s = fabsf(d[0]) + fabsf(d[1]);
    if constexpr (DIM == 3) s += fabsf(d[2]);
    return s;
}
template <int DIM>
__device__ __forceinline__ wf_f2 wf_l1(const wf_f2 (&d)[DIM]) {          // per half: v_add_f32 takes |.| as a source modifier
    float sx = fabsf(d[0].x) + fabsf(d[1].x), sy = fabsf(d[0].y) + fabsf(d[1].y);
    if constexpr (DIM == 3) { sx += fabsf(d[2].x); sy += fabsf(d[2].y); }
    return wf_f2{sx, sy};
}

// acc + ((x - q) . an) / dist(x - q)^POWER for the one or two queries of V
template <int DIM, int METRIC, int POWER, typename V>
__device__ __forceinline__ V wf_add(const float (&x)[DIM], const float (&an)[DIM], const V (&q)[DIM], V acc) {
    V d[DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) d[i] = x[i] - q[i];
    V num = d[0] * an[0];
#pragma unroll
    for (int i = 1; i < DIM; ++i) num = wf_fma(d[i], V(an[i]), num);
    V inv;
    if constexpr (METRIC == 0) {
        const V s = wf_l1<DIM>(d);
        V sp = s * s;
        if constexpr (POWER == 3) sp *= s;
        inv = wf_rcp(sp);
    } else {
        V r2 = d[0] * d[0];
#pragma unroll
        for (int i = 1; i < DIM; ++i) r2 = wf_fma(d[i], d[i], r2);
        const V rs = wf_rsq(r2);
        inv = rs * rs;
        if constexpr (POWER == 3) inv *= rs;
    }
    return wf_fma(num, inv, acc);
}

__device__ __forceinline__ float wf_lane(float v, int) { return v; }
__device__ __forceinline__ float wf_lane(wf_f2 v, int l) { return l ? v.y : v.x; }
__device__ __forceinline__ void wf_set(float& v, int, float s) { v = s; }
__device__ __forceinline__ void wf_set(wf_f2& v, int l, float s) { if (l) v.y = s; else v.x = s; }

// points, normals: (B, npts, DIM); area: (B, npts) or null; queries: (DIM, nq); out: (B, nq) or null; mask: (B, nq) or null
template <int DIM, int METRIC, int POWER, int Q>
__global__ void __launch_bounds__(WF_THREADS) winding_field_kernel(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                                   const float* __restrict__ area, const float* __restrict__ queries,
                                                                   float* __restrict__ out, uint8_t* __restrict__ mask, int npts,
                                                                   int64_t nq, float scale, float threshold) {
    constexpr int L = Q == 1 ? 1 : 2;                   // queries per register (pair)
    using V = typename std::conditional<L == 1, float, wf_f2>::type;
    constexpr int NV = Q / L;
    __shared__ float4 sa[WF_CHUNK];                     // 2-D: (x, y, nx a, ny a);  3-D: (x, y, z, nx a)
    __shared__ float2 sb[DIM == 3 ? WF_CHUNK : 1];      // 3-D: (ny a, nz a)
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int64_t q0 = (int64_t)blockIdx.x * (WF_THREADS * Q) + tid;
    V qc[NV][DIM], acc[NV];
#pragma unroll
    for (int k = 0; k < Q; ++k) {                       // query k of the thread: half k % L of vector k / L
        const int64_t qk = q0 + (int64_t)k * WF_THREADS;
        const int64_t q = qk < nq ? qk : nq - 1;                             // past the end: a copy of the last query, never stored
#pragma unroll
        for (int i = 0; i < DIM; ++i) wf_set(qc[k / L][i], k % L, queries[(int64_t)i * nq + q]);
        wf_set(acc[k / L], k % L, 0.f);
    }
    const size_t pbase = (size_t)b * (size_t)npts;
    for (int p0 = 0; p0 < npts; p0 += WF_CHUNK) {
        const int cnt = min(WF_CHUNK, npts - p0);
        if (tid < cnt) {
            const size_t p = pbase + (size_t)(p0 + tid);
            const float a = area ? area[p] : 1.0f;
            float x[DIM], an[DIM];
#pragma unroll
            for (int i = 0; i < DIM; ++i) {
                x[i] = pts[p * DIM + i];
                an[i] = nrm[p * DIM + i] * a;
            }
            if constexpr (DIM == 2) {
                sa[tid] = make_float4(x[0], x[1], an[0], an[1]);
            } else {
                sa[tid] = make_float4(x[0], x[1], x[2], an[0]);
                sb[tid] = make_float2(an[1], an[2]);
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < cnt; ++j) {
            const float4 va = sa[j];
            float x[DIM], an[DIM];
            if constexpr (DIM == 2) {
                x[0] = va.x; x[1] = va.y; an[0] = va.z; an[1] = va.w;
            } else {
                const float2 vb = sb[j];
                x[0] = va.x; x[1] = va.y; x[2] = va.z; an[0] = va.w; an[1] = vb.x; an[2] = vb.y;
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) acc[k] = wf_add<DIM, METRIC, POWER, V>(x, an, qc[k], acc[k]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        const int64_t q = q0 + (int64_t)k * WF_THREADS;
        if (q < nq) {
            const float w = scale * wf_lane(acc[k / L], k % L);
            const size_t o = (size_t)b * (size_t)nq + (size_t)q;
            if (out) out[o] = w;
            if (mask) mask[o] = w > threshold ? 1 : 0;
        }
    }
}

using WfKernel = void (*)(const float*, const float*, const float*, const float*, float*, uint8_t*, int, int64_t, float, float);

template <int Q>
static WfKernel wf_pick(int dim, int metric, int power) {
    const int key = (dim - 2) * 4 + metric * 2 + (power - 2);
    switch (key) {
        case 0: return winding_field_kernel<2, 0, 2, Q>;
        case 1: return winding_field_kernel<2, 0, 3, Q>;
        case 2: return winding_field_kernel<2, 1, 2, Q>;
        case 3: return winding_field_kernel<2, 1, 3, Q>;
        case 4: return winding_field_kernel<3, 0, 2, Q>;
        case 5: return winding_field_kernel<3, 0, 3, Q>;
        case 6: return winding_field_kernel<3, 1, 2, Q>;
        default: return winding_field_kernel<3, 1, 3, Q>;
    }
}

}  // namespace dn

// Queries per thread for a problem: the largest tile that still leaves every SIMD of the chip (256 CUs x 4) about four waves,
// batch * nq / (64 Q) >= 4096; below that a larger tile only idles SIMDs (25^3 probes x 10 242 points: 534 / 619 / 888 us at
// Q = 1 / 2 / 4; 128^3 nodes: 5.45 / 5.43 / 5.19 ms; profiles/winding_field.txt).
extern "C" int dn_winding_field_tile(int32_t batch, int64_t nq) {
    if (batch < 1 || nq < 1) return DN_E_BADARG;
    const int64_t total = (int64_t)batch * nq;
    return total >= (int64_t)4 * 64 * 4096 ? 4 : total >= (int64_t)2 * 64 * 4096 ? 2 : 1;
}

extern "C" int dn_winding_field(const float* points, const float* normals, const float* area, const float* queries, float* out,
                                uint8_t* mask, int32_t batch, int32_t npts, int64_t nq, int32_t dim, int32_t metric, int32_t power,
                                float scale, float threshold, int32_t tile, void* stream) {
    if (!points || !normals || !queries || (!out && !mask)) return DN_E_BADARG;
    if (dim != 2 && dim != 3) return DN_E_BADARG;
    if (power != 2 && power != 3) return DN_E_BADARG;
    if (metric != 0 && metric != 1) return DN_E_BADARG;
    if (tile != 0 && tile != 1 && tile != 2 && tile != 4) return DN_E_BADARG;
    if (batch < 1 || batch > 65535 || npts < 1 || nq < 1) return DN_E_BADARG;
    const int q = tile ? tile : dn_winding_field_tile(batch, nq);
    const int64_t w = (int64_t)dn::WF_THREADS * q;
    if (nq > dn::WF_MAX_BLOCKS * w) return DN_E_BADARG;
    const int64_t blocks = (nq + w - 1) / w;
    const dn::WfKernel k = q == 4 ? dn::wf_pick<4>(dim, metric, power) : q == 2 ? dn::wf_pick<2>(dim, metric, power) : dn::wf_pick<1>(dim, metric, power);
    hipLaunchKernelGGL(k, dim3((unsigned)blocks, (unsigned)batch), dim3(dn::WF_THREADS), 0, reinterpret_cast<hipStream_t>(stream), points,
                       normals, area, queries, out, mask, (int)npts, nq, scale, threshold);
    DN_LAUNCH_CHECK();
    return 0;
}
