// 2-D Q1 fused Poisson kernel, closed-form element (the default for nodal / absent forcing).
//
// With u, nu, f bilinear on the element, every quadrature sum of the reference's loss bodies is a polynomial in the lerp coordinates
// b_g in [0, 1] of the 1-D Gauss points summed against the rule, i.e. a combination of the rule's moments  sum_g w_g (1 - b_g)^r b_g^s.
// Stiffness term, symmetric in the layer's lower (L) and upper (U) node row (q1cf_stage / q1cf_elem in poisson_elem.h): per node row and
// element the kernel stages  du[e] = u[e + 1] - u[e]  and the x-moment of nu  pn[e] = sum_i wx_i nu(x_i)  ONCE, when the row lands (each
// row is the upper row of one layer and the lower row of the next); a layer then needs, with a = du_L, b = du_U, p = pn_L, q = pn_U,
//     sum_g W nu u_x^2 = hs0^2 ( a^2 (p r30 + q r21) + 2 a b (p r21 + q r12) + b^2 (p r12 + q r03) ),   r_rs = sum_g w_g (1 - b_g)^r b_g^s,
// and the same cubic in the per-node vertical differences V[n] = u_U[n] - u_L[n] and y-moments S[n] of nu for the y-derivative.  hs^2
// and the user scale are folded into the r_rs on the host (ElemTab::q1xm / q1ym, in double); alpha enters where the cotangents are added to
// the nodes (an FMA in place of an add), so the energy sums need no division and alpha = 0 is as good as any.  Forcing term:  sum_g W f N_a = (mass_x (x) mass_y) f, applied axis by axis (fstage / layer).
// This is algebra, not a change of rule: the moments are computed from the rule's own points and weights (including the reference's
// truncated 3- and 4-point literals), so the value equals the Gauss sum over any ngp x ngp points to rounding
// (tests/test_q1cf_rowstaged.py: 1e-12 in float64).  Main loop of the bench instantiation <4, true, nu | f | one bit-packed condition, 1>,
// two node rows = eight elements per thread: 569 VALU instructions, 16 loads, 2 stores, 2 barriers, 100 VGPRs (552 and 98 before the shared
// node came from the neighbouring lane, profiles/q1cf_cache_policy.txt; the element on raw nodal values: 724 and 105; tools/q1cf_loop_count.py,
// profiles/q1cf_rowstaged.txt).  The generic mask / value-field form (CF_BC)
// keeps the element on raw nodal values (ROWSTAGED below).
//
// Mapping as the other 2-D kernels: a thread owns E consecutive elements of a strip and marches over element rows; it
// carries the lower node row (raw nodal values) and the layer-below contributions to that row's nodes; two rows per loop
// trip with the two raw rows / carry sets swapping roles (no copies); node shared with the right neighbour through LDS.
#include <cstdlib>
#include <type_traits>

#define DN_NT_STORES 1            // the gradient rows are written once and never re-read by the launch: 54.3 -> 52.8 us when every load was plain
                                  // (profiles/r2_ab2d_nt.txt); with today's non-temporal loads, on the rotation: plain stores 58.7-59.2 us, write-through
                                  // (sc1) 58.6-58.9, non-temporal 55.3-55.9 -- and 56.3-57.9 / 55.4-57.0 / 51.5-51.7 with the shared node from the
                                  // neighbouring lane and non-temporal u (profiles/q1cf_cache_policy.txt).  The flat-stream probe's ranking (plain ahead) does not carry over
#include "poisson_common.h"

namespace dn {

// CF_BC_PACKED: bit-packed masks / box faces with constant values; CF_PK_NB1 / CF_PK_NB2: one / two of the conditions are bit arrays
// (compile-time: a load inside a wave-uniform branch costs an s_waitcnt vmcnt(0) where the branch joins)
// CF_ONE (packed and uint8-constant masks): exactly one condition is present -- the absent one costs no bit test, compare or select
enum : int { CF_NU = 1, CF_F = 2, CF_BC = 8, CF_BC_U8C = 16, CF_BC_PACKED = 32, CF_PK_NB1 = 64, CF_PK_NB2 = 128, CF_UA = 256, CF_ONE = 512 };
// CF_UA (E = 4, vector accesses, one strip per workgroup): rows of 4 k + 1 nodes -- the 2^n + 1 meshes.  The 16-byte row accesses are then aligned to 4 bytes
// only (the hardware takes that), and the mesh's LAST node column belongs to the last full thread column (its node x0 + 4) instead of to a thread column of
// its own: the launch has the geometry of the 4 k mesh (513^2 x 64: 112.9 -> the time of 512^2, tools/time_2d_sizes.py).

template <int E>
struct CfRow {
    float u[E + 1], n[E + 1], f[E + 1];
    float g[E + 1];          // x-stage of the forcing term: (1-D element mass matrix in x) applied to f over the thread's own elements
    float du[E], pn[E];      // x-stage of the stiffness term (q1cf_stage): u[e + 1] - u[e] and the x-moment of nu over element e
    float keep[E];
    float keepx;             // CF_UA: keep of the node x0 + E (the mesh's last node column in the last thread column)
    BcRaw<E> bc;
    uint32_t m8[2][2];
    uint32_t mb[2];          // CF_BC_PACKED: bits of the row's nodes x0, x0 + 1, ... from the bit arrays (bit n = node x0 + n)
    uint32_t bx[2];          //                 box-face bits of those nodes, per condition
};

// Measured and removed (code in the history):
//  - the shared node x0 + 4 from the neighbouring lane, exchanged when the row is ISSUED: over DPP equal (profiles/r2_2d_ab.txt), over ds_bpermute
//    with non-temporal row loads slower, 60-69 us -- every row load waited for the one before.  Exchanged when the row has
//    LANDED it is what the kernel does now (XCH below)
//  - plain or write-through (sc1) stores of the gradient rows in place of non-temporal ones: +3 us without, +4 to +6 us with the lane exchange;
//    u's loads non-temporal on the rows a neighbouring strip reads as well: +0.6 to +1.0 us (profiles/q1cf_cache_policy.txt)
//  - neighbouring strips marching in opposite directions on one XCD: traffic 1.09x -> 1.002x of the algorithmic bytes, but slower where every
//    launch streams from HBM (59.5 vs 56.4 us, profiles/r2_rotate_variants.txt)
//  - software-pipelined rows (one / two raw rows in flight): 48.1 / 50.6 us against 46.9 on the default plan (profiles/r2_plan2d_steady.txt)
//  - element pairs in packed fp32 registers: 722 -> 536 VALU instructions per two rows, 105 -> 154 VGPRs, no gain (profiles/r3_2d_packed.txt)
constexpr int CF_W = 4;           // sub-strips CHAINED per workgroup where the launch plan asks for it ("PLAN2D" "T,E,R,W"; not the default, see plan2d in
                                  // poisson_fused.hip): W x 2 waves march W neighbouring strips; a strip takes the row it shares with the strip below / above
                                  // through LDS instead of re-reading it from HBM and recomputing the seam layer: a workgroup of W strips of R rows reads
                                  // W R + 2 rows instead of W (R + 2)
constexpr int CF_TS = 128;        // threads per chained sub-strip (two waves: 128 x 4 elements = one 512-node row segment)
constexpr int CF_NSLOT = 64;      // hand-over slots between the two waves of a sub-strip: one per emitted row, never reused (R + 3 <= 64)
constexpr unsigned CF_SPIN_MAX = 1u << 20;   // bound of every LDS flag poll: a producer wave that never arrives must not hang the GPU.  Reaching the bound is NOT
                                             // silent: the wave poisons everything it writes afterwards with NaN (output rows, its partial sums -> the
                                             // launch's energy / sumsq are NaN) and sets the sticky error word of the workspace header (dn_workspace_status)

// LDS hand-overs of the chained strips are spelled as inline asm: a `volatile` LDS access makes the compiler wait for EVERY outstanding
// memory operation around it (s_waitcnt vmcnt(0) lgkmcnt(0): 237 of them in the first build of the chained kernel, i.e. the row loads
// no longer overlapped anything, +5 us per launch).  The asm forms touch lgkmcnt only; LDS returns a wave's accesses in order.
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)p; }
__device__ __forceinline__ void lds_st(unsigned a, float v) { asm volatile("ds_write_b32 %0, %1" ::"v"(a), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_st(unsigned a, unsigned v) { asm volatile("ds_write_b32 %0, %1" ::"v"(a), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_ld_nowait(float& d, unsigned a) { asm volatile("ds_read_b32 %0, %1" : "=v"(d) : "v"(a) : "memory"); }
__device__ __forceinline__ unsigned lds_ld_u(unsigned a) {
    unsigned d;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(d) : "v"(a) : "memory");
    return d;
}
__device__ __forceinline__ float lds_ld(unsigned a) {
    float d;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(d) : "v"(a) : "memory");
    return d;
}
// after a group of lds_ld_nowait: the wait, tied to the destinations so that no use of them is scheduled above it
template <int N>
__device__ __forceinline__ void lds_wait(float (&v)[N]) {
    if constexpr (N == 5) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4])::"memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3])::"memory");
    else if constexpr (N == 3) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2])::"memory");
    else if constexpr (N == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1])::"memory");
    else { static_assert(N == 1, "lds_wait: 1..5 values"); asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0])::"memory"); }
}

template <int E, bool VEC, int FL, int W>
__global__ void __launch_bounds__(W > 1 ? CF_TS * W : 256, W > 1 ? 4 : 2) poisson2d_q1_cf_kernel(const PoissonParams p) {
    constexpr int NW = E;
    constexpr bool HAS_NU = (FL & CF_NU) != 0, HAS_F = (FL & CF_F) != 0;
    constexpr bool BC_ANY = (FL & (CF_BC | CF_BC_U8C | CF_BC_PACKED)) != 0, BC_U8C = (FL & CF_BC_U8C) != 0, BC_PACKED = (FL & CF_BC_PACKED) != 0;
    constexpr bool UA = (FL & CF_UA) != 0, ONE = (FL & CF_ONE) != 0;
    static_assert(!ONE || ((BC_PACKED || BC_U8C) && (FL & CF_PK_NB2) == 0), "CF_ONE: one packed or uint8-constant condition");
    static_assert(!UA || (E == 4 && VEC && W == 1), "CF_UA: four elements per thread, vector accesses, one strip per workgroup");
    // W > 1: the workgroup holds W sub-strips of CF_TS threads each; sub (wave-uniform) is this thread's sub-strip
    const int T = W > 1 ? CF_TS : (int)blockDim.x;
    const int sub = W > 1 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / CF_TS) : 0;       // wave-uniform: everything derived from it stays scalar
    const int tid = W > 1 ? (int)threadIdx.x - sub * CF_TS : (int)threadIdx.x;
    const int chunk = blockIdx.x, strip = W > 1 ? (int)blockIdx.y * W + sub : selected_strip(p, (int)blockIdx.y), b = blockIdx.z;      // (chained launches cover every strip)
    const bool active = W == 1 || strip < p.nstrips;                         // the last workgroup of a sample may hold fewer than W strips
    const bool chain_dn = W > 1 && sub > 0;                                  // the strip below is in this workgroup
    const bool chain_up = W > 1 && sub + 1 < W && strip + 1 < p.nstrips;     // the strip above is
    const int q = chunk * (T - 1) + tid;  // logical thread column (chunks overlap by one thread)
    const int ex0 = q * E;
    const int x0 = ex0;
    const bool col_owner = !(chunk > 0 && tid == 0);
    const bool lastcol = UA && x0 + NW == p.nx - 1;      // this thread's shared node is the mesh's last node column: nobody to the right owns it
    // XCH (four elements per thread, one strip per workgroup; not the generic mask / value-field form, which it would push from 4 to 3
    // waves per SIMD): the node x0 + NW of u, nu and f comes from the right neighbour's lane once the row has landed (row_bc) instead of
    // from a strided dword load per lane.  has_nb: the neighbour is a lane of this wave; every other lane -- lane 63, the chunk's last
    // thread, the CF_UA thread whose shared node is the mesh's last column -- keeps its own load (xs: load_seg4_xs)
    constexpr bool XCH = W == 1 && VEC && E == 4 && (FL & CF_BC) == 0;
    const bool has_nb = XCH && ((int)threadIdx.x & 63) < 63 && (int)threadIdx.x + 1 < (int)blockDim.x && !lastcol;
    const unsigned xs = (unsigned)min((has_nb ? __builtin_amdgcn_readfirstlane(q) + 63 : q) * E + NW, p.nx - 1);
    const int64_t nps = (int64_t)p.nx * p.ny;
    const SampleBases sb = sample_bases(p, b, nps);
    const int R = p.rows_per_strip;
    // The strip owns the node rows [sb0, sc0) (the last strip also the top row of the domain) and the element layers between them; it
    // also computes the layer below its first row (the seam: that row's other half), so it reads the node rows sb0 - 1 .. sc0.
    const int sb0 = strip * R, sc0 = min(sb0 + R, p.nely);
    // layers [ey_begin, ey_end); energy counted for layers e_from <= ey <= e_until, rows stored for ey >= r_from
    const int ey_begin = (sb0 > 0 && !chain_dn) ? sb0 - 1 : sb0;          // chain_dn: no seam layer, the carry comes from the strip below
    const int ey_end = sc0;
    const int r_from = sb0;
    const int e_from = sb0, e_until = p.nely;
    const bool top_row = sc0 == p.nely;                                      // the strip also finishes the last row (no layer above it)

    __shared__ float xch[2][256];
    __shared__ double red[W > 1 ? 4 * W : 8];
    __shared__ int last_flag;
    // W > 1 -- hand-overs inside the workgroup, all through LDS words guarded by flags (no workgroup barrier: the sub-strips, and the two
    // waves of a sub-strip, run at their own pace; a producer never waits for a consumer, so there is no cycle of waits):
    //   cf_edge / cf_xflag   per emitted row, wave 0 of a sub-strip -> wave 1: the contribution to the node the two waves share
    //   cf_seam / cf_sflag   once per strip: the strip above publishes its first node row (Dirichlet applied, forcing x-staged) for the
    //                        last layer of the strip below [0 .. 3 NW + 2]; the strip below answers with that layer's contributions
    //                        to this row [3 NW + 3 .. 4 NW + 3]; the strip above parks its own half of the row meanwhile [4 NW + 4 ..]
    constexpr int CW = W > 1 ? W : 2, SEAM_WORDS = 6 * (E + 1);
    __shared__ float cf_edge[W > 1 ? W : 1][W > 1 ? CF_NSLOT : 1];
    __shared__ unsigned cf_xflag[W > 1 ? W : 1];
    __shared__ float cf_seam[CW - 1][W > 1 ? SEAM_WORDS : 1][W > 1 ? CF_TS : 1];
    __shared__ unsigned cf_sflag[CW - 1][2][2];          // [seam][0: row published, 1: carry published][wave of the sub-strip]
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned seq = 0u;                                   // rows handed over so far (same count in both waves of a sub-strip)
    if constexpr (W > 1) {
        static_assert(CF_TS == 128, "two waves per sub-strip");
        if (threadIdx.x < (unsigned)W) cf_xflag[threadIdx.x] = 0u;
        if (threadIdx.x < 4u * (W - 1)) (&cf_sflag[0][0][0])[threadIdx.x] = 0u;
        __syncthreads();
    }
    // dn_poisson_args.fold_prev: the launch's first workgroup closes the evaluation before it (1-2 us once per launch, off every critical path)
    if ((blockIdx.x | blockIdx.y | blockIdx.z) == 0u) fold_prev_sums(p, (int)threadIdx.x, (int)blockDim.x, red);
    float spin_poison = 0.f;                                              // NaN once a poll has run into its bound (wave-uniform)
    auto spin_until = [&](const unsigned* flag, unsigned want) {          // wave-uniform poll of an LDS word
        const unsigned fa = lds_addr(flag);
        const unsigned lim = p.spin_limit > 0 ? (unsigned)p.spin_limit : CF_SPIN_MAX;
        unsigned n = 0;
        for (; n < lim; ++n) {
            if ((unsigned)__builtin_amdgcn_readfirstlane((int)lds_ld_u(fa)) >= want) break;
            __builtin_amdgcn_s_sleep(1);
        }
        if (n == lim) spin_poison = __builtin_nanf("");
    };

    const bool has_mask[2] = {sb.mask[0] != nullptr, sb.mask[1] != nullptr};
    const uint8_t* mask8[2];
    mask8[0] = reinterpret_cast<const uint8_t*>(has_mask[0] ? sb.mask[0] : sb.mask[1]);
    mask8[1] = reinterpret_cast<const uint8_t*>(has_mask[1] ? sb.mask[1] : sb.mask[0]);

    // CF_BC_PACKED: per condition either one bit per node in HBM (one 2-byte load per thread, row and bit array) or the domain faces
    // (no load).  Branch-free: NB loads are always issued; what a condition contributes is selected with wave-uniform masks.
    constexpr unsigned NBITS = (1u << (NW + 1)) - 1u;
    constexpr int NB = !BC_PACKED ? 0 : ((FL & CF_PK_NB2) ? 2 : ((FL & CF_PK_NB1) ? 1 : 0));
    const bool isbits[2] = {p.bc[0].kind == DN_MASK_BITS, p.bc[1].kind == DN_MASK_BITS};
    const unsigned bsel[2] = {isbits[0] ? NBITS : 0u, isbits[1] ? NBITS : 0u};
    // load slot j reads the bit array of condition src[j]; with one array it is whichever condition has it
    const int src0 = (NB == 2 || isbits[0]) ? 0 : 1;
    const int kone = p.bc[0].kind >= 0 ? 0 : 1;                // CF_ONE: the condition that is present
    const uint32_t* bptr[2] = {reinterpret_cast<const uint32_t*>(sb.mask[src0]), reinterpret_cast<const uint32_t*>(sb.mask[1])};
    // two ALIGNED dwords per bit array and row (the word that holds node x0 and the next one; 8 lanes share an address) and one
    // v_alignbit: an unaligned 2-byte window costs the address path 16 cycles per wave-instruction, an aligned dword 4.5
    const unsigned brow[2] = {(unsigned)p.bc[src0].row_bytes / 4u, (unsigned)p.bc[1].row_bytes / 4u};       // words per node row
    unsigned bw0[2], bw1[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int rw = max((int)brow[j], 1);
        bw0[j] = (unsigned)min(x0 >> 5, rw - 1);
        bw1[j] = (unsigned)min((x0 >> 5) + 1, rw - 1);
    }
    const unsigned bsh = (unsigned)x0 & 31u;
    unsigned boxx[2] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int faces = p.bc[k].kind == DN_MASK_BOX ? p.bc[k].box_faces : 0;
#pragma unroll
        for (int n = 0; n <= NW; ++n) {
            const bool on = ((faces & DN_FACE_XLO) && x0 + n == 0) || ((faces & DN_FACE_XHI) && x0 + n == p.nx - 1);
            boxx[k] |= on ? (1u << n) : 0u;
        }
    }
    const int ylo[2] = {(p.bc[0].kind == DN_MASK_BOX && (p.bc[0].box_faces & DN_FACE_YLO)) ? 0 : -1,
                        (p.bc[1].kind == DN_MASK_BOX && (p.bc[1].box_faces & DN_FACE_YLO)) ? 0 : -1};
    const int yhi[2] = {(p.bc[0].kind == DN_MASK_BOX && (p.bc[0].box_faces & DN_FACE_YHI)) ? p.ny - 1 : -1,
                        (p.bc[1].kind == DN_MASK_BOX && (p.bc[1].box_faces & DN_FACE_YHI)) ? p.ny - 1 : -1};
    auto packed_issue = [&](int yc, CfRow<E>& r) {                   // yc: node row, already clamped into the mesh
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const unsigned ro = (unsigned)yc * brow[j];
            const uint32_t w0 = ld_at<uint32_t>(bptr[j], ro + bw0[j]), w1 = ld_at<uint32_t>(bptr[j], ro + bw1[j]);
            r.mb[j] = __builtin_amdgcn_alignbit(w1, w0, bsh);          // bit n = node x0 + n
        }
        if constexpr (ONE) {
            if constexpr (NB == 0) r.bx[0] = (yc == (kone ? ylo[1] : ylo[0]) || yc == (kone ? yhi[1] : yhi[0])) ? NBITS : (kone ? boxx[1] : boxx[0]);
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) r.bx[k] = (yc == ylo[k] || yc == yhi[k]) ? NBITS : boxx[k];
        }
    };

    // nt_u (XCH): u's vector load non-temporal
    auto row_issue = [&](auto nt_u, int yr, CfRow<E>& r) {
        const int yp = min(yr, p.ny - 1);
        const unsigned rowoff = (unsigned)yp * (unsigned)p.nx;
        // nu and f (read once per launch) as non-temporal vector loads.  On one re-evaluated batch this gives up the Infinity-Cache hits
        // (47 -> 53 us); on batches in rotation -- every launch streams from HBM, the regime bench.py times -- it wins: mask bits 58.3 -> 55.5 us,
        // box 56.5 -> 56.0 (profiles/r3_rotate_nt.txt).  u as well was slower (59.8) as long as every lane re-read its shared node with a dword
        // load; with the shared node taken from the neighbouring lane (XCH) the rotation goes 55.5 -> 52.8 us with plain u loads,
        // -> 51.6 with non-temporal ones on every row and -> 50.3 (against 51.2 in that series) with the rows a neighbouring strip reads
        // as well kept plain (nt_u, see the march below; profiles/q1cf_cache_policy.txt)
        if constexpr (XCH) {
            load_seg4_xs<decltype(nt_u)::value>(sb.u, rowoff, x0, p.nx, xs, r.u);
            if constexpr (HAS_NU) load_seg4_xs<true>(sb.nu, rowoff, x0, p.nx, xs, r.n);
            if constexpr (HAS_F) load_seg4_xs<true>(sb.f, rowoff, x0, p.nx, xs, r.f);
        } else {
            load_seg<NW, VEC>(sb.u, rowoff, x0, p.nx, r.u);
            if constexpr (HAS_NU) load_seg_stream<NW, VEC>(sb.nu, rowoff, x0, p.nx, r.n);
            if constexpr (HAS_F) load_seg_stream<NW, VEC>(sb.f, rowoff, x0, p.nx, r.f);
        }
        if constexpr (BC_PACKED) {
            packed_issue(yp, r);
        } else if constexpr (BC_U8C && ONE) {
            uint8_t t[NW + 1];
            load_seg_stream<NW, VEC>(mask8[0], rowoff, x0, p.nx, t);          // mask8[0]: the image of the condition that is present
            uint32_t w = 0u;
#pragma unroll
            for (int n = 0; n < NW; ++n) w |= (uint32_t)t[n] << (8 * n);
            r.m8[0][0] = w;
            r.m8[0][1] = t[NW];
        } else if constexpr (BC_U8C) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (has_mask[k]) {                    // an absent condition costs no load (wave-uniform branch)
                    uint8_t t[NW + 1];
                    load_seg_stream<NW, VEC>(mask8[k], rowoff, x0, p.nx, t);
                    uint32_t w = 0u;
#pragma unroll
                    for (int n = 0; n < NW; ++n) w |= (uint32_t)t[n] << (8 * n);
                    r.m8[k][0] = w;
                    r.m8[k][1] = t[NW];
                }
            }
        } else if constexpr (BC_ANY) {
            bc_issue<NW, VEC>(p, sb, rowoff, x0, r.bc);
        }
    };
    // u <- where(mask, value, u) on a landed row, keep[] = 0 on its Dirichlet nodes; before that (XCH) the row's shared nodes, as they
    // landed: every thread applies the conditions to its five nodes itself, from its own mask bits
    auto row_bc = [&](CfRow<E>& r) {
        if constexpr (XCH) {
            seg_take_shared(r.u, has_nb);
            if constexpr (HAS_NU) seg_take_shared(r.n, has_nb);
            if constexpr (HAS_F) seg_take_shared(r.f, has_nb);
        }
#pragma unroll
        for (int n = 0; n < NW; ++n) r.keep[n] = 1.f;
        if constexpr (UA) r.keepx = 1.f;
        if constexpr ((BC_PACKED || BC_U8C) && ONE) {
            const float v = kone ? p.bc[1].value : p.bc[0].value;
            unsigned b = 0u;
            if constexpr (BC_PACKED) b = NB == 1 ? r.mb[0] : r.bx[0];      // (one condition: a bit array or box faces)
#pragma unroll
            for (int n = 0; n <= NW; ++n) {
                bool set;
                if constexpr (BC_PACKED) set = (b & (1u << n)) != 0u;
                else set = n < NW ? ((r.m8[0][0] >> (8 * n)) & 0xffu) != 0u : r.m8[0][1] != 0u;
                r.u[n] = set ? v : r.u[n];
                if (n < NW) r.keep[n] = set ? 0.f : 1.f;
                else if constexpr (UA) r.keepx = set ? 0.f : 1.f;
            }
        } else if constexpr (BC_PACKED) {
            unsigned b0 = r.bx[0], b1 = r.bx[1];
            if constexpr (NB == 2) { b0 |= r.mb[0] & bsel[0]; b1 |= r.mb[1] & bsel[1]; }
            if constexpr (NB == 1) { b0 |= r.mb[0] & bsel[0]; b1 |= r.mb[0] & bsel[1]; }
            const float v0 = p.bc[0].value, v1 = p.bc[1].value;
#pragma unroll
            for (int n = 0; n <= NW; ++n) {
                r.u[n] = (b0 & (1u << n)) ? v0 : r.u[n];
                r.u[n] = (b1 & (1u << n)) ? v1 : r.u[n];
                if (n < NW) r.keep[n] = ((b0 | b1) & (1u << n)) ? 0.f : 1.f;
            }
            if constexpr (UA) r.keepx = ((b0 | b1) & (1u << NW)) ? 0.f : 1.f;
        } else if constexpr (BC_U8C) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (has_mask[k]) {
                    const float val = p.bc[k].value;
#pragma unroll
                    for (int n = 0; n <= NW; ++n) {
                        const bool set = has_mask[k] && (n < NW ? ((r.m8[k][0] >> (8 * n)) & 0xffu) != 0u : r.m8[k][1] != 0u);
                        r.u[n] = set ? val : r.u[n];
                        if (n < NW) r.keep[n] = set ? 0.f : r.keep[n];
                        else if constexpr (UA) r.keepx = set ? 0.f : r.keepx;
                    }
                }
            }
        } else if constexpr (BC_ANY) {
            if constexpr (UA) {
                float k5[NW + 1];
                bc_apply_all<NW>(p, sb, r.bc, r.u, k5);
#pragma unroll
                for (int n = 0; n < NW; ++n) r.keep[n] = k5[n];
                r.keepx = k5[NW];
            } else {
                bc_apply<NW>(p, sb, r.bc, r.u, r.keep);
            }
        }
    };

    float e1_acc = 0.f, e2_acc = 0.f, sq_acc = 0.f;
    int par = 0;

    // emit_row stages the finished row in pend_* and writes it through flush_store().  (The software-pipelined march, since removed, used
    // the staging to issue the store after the next row's loads: a store in a divergent branch that is younger than the loads the next
    // consumer waits for turns that wait into vmcnt(0), i.e. into a wait for the store itself.)
    float pend_v[NW];
    unsigned pend_row = 0u;
    bool pend_st = false;
    float pend_x = 0.f;          // CF_UA: the last node column's value (last thread column)
    auto flush_store = [&]() {
        if (pend_st) store_seg<NW, VEC>(sb.out, pend_row, x0, p.nx, pend_v);
        if constexpr (UA) {
            if (pend_st && lastcol) st_at<float>(sb.out, pend_row + (unsigned)(p.nx - 1), pend_x);
        }
        pend_st = false;
    };
    auto emit_row = [&](const float (&o)[NW + 1], const float (&keep)[NW], int yr, bool owned_row, float keepx = 1.f) {
        float left;
        if constexpr (W > 1) {
            // inside a wave: lane l takes o[NW] of lane l - 1 (ds_bpermute); across the two waves: one LDS word per row + a row counter
            const float up = __shfl_up(o[NW], 1, 64);
            const unsigned ea = lds_addr(&cf_edge[sub][seq & (CF_NSLOT - 1)]);
            float edge = 0.f;
            if (wv == 0) {
                if (lane == 63) { lds_st(ea, o[NW]); lds_st(lds_addr(&cf_xflag[sub]), seq + 1u); }     // LDS executes a wave's accesses in order: value before counter
            } else {
                spin_until(&cf_xflag[sub], seq + 1u);
                edge = lds_ld(ea);
            }
            left = lane > 0 ? up : edge;
            ++seq;
        } else {
            xch[par][tid] = o[NW];
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // LDS-only barrier (loads stay in flight)
            left = (tid > 0) ? xch[par][tid - 1] : 0.f;
            par ^= 1;
        }
        // (CF_UA: the thread column right of the last full one receives the last node column's contribution over the hand-over, but does not own it)
        const bool st = owned_row && col_owner && (!UA || x0 + NW <= p.nx - 1);
#pragma unroll
        for (int n = 0; n < NW; ++n) {
            const float t = (o[n] + (n == 0 ? left : 0.f)) * keep[n];
            sq_acc = st ? fmaf(t, t, sq_acc) : sq_acc;       // nodes beyond the domain receive no contribution: t == 0
            pend_v[n] = t * p.out_scale;
            if constexpr (W > 1) pend_v[n] += spin_poison;
        }
        if constexpr (UA) {               // the mesh's last node column: finished by the thread column left of it (no thread to hand it to)
            const float t = o[NW] * keepx;
            sq_acc = (st && lastcol) ? fmaf(t, t, sq_acc) : sq_acc;
            pend_x = t * p.out_scale;
        }
        pend_row = (unsigned)yr * (unsigned)p.nx;
        pend_st = st && sb.out != nullptr;
        flush_store();
    };

    const float mx0 = p.T.mxs[0], mx1 = p.T.mxs[1], mx2 = p.T.mxs[2], mx3 = p.T.mxs[3];
    const float my0 = p.T.m[0], my1 = p.T.m[1], my2 = p.T.m[2], my3 = p.T.m[3];
    const float k0 = p.T.q1c[0], k1 = p.T.q1c[1], h0 = p.T.q1c[2], h1 = p.T.q1c[3], nb = -p.T.beta;
    // ROWSTAGED: the stiffness term from quantities staged once per node row (q1cf_stage / q1cf_elem, poisson_elem.h), hs^2 folded into the
    // moment constants on the host (ElemTab); alpha enters where the cotangents are added to the nodes.  Every form but the generic mask / value-field one (CF_BC),
    // which keeps the element on raw nodal values: its register budget is at the edge of 4 waves per SIMD as it is.
    // STAGE_DU: du[] kept per row; the chained strips (W > 1, 13 more VGPRs for the hand-overs) keep pn[] only and recompute the differences
    constexpr bool ROWSTAGED = (FL & CF_BC) == 0, STAGE_DU = W == 1;
    const float xm[4] = {p.T.q1xm[0], p.T.q1xm[1], p.T.q1xm[2], p.T.q1xm[3]}, ym[4] = {p.T.q1ym[0], p.T.q1ym[1], p.T.q1ym[2], p.T.q1ym[3]};
    const float px0 = p.T.q1px[0], px1 = p.T.q1px[1], sy0 = p.T.q1sy[0], sy1 = p.T.q1sy[1];

    // forcing term as a tensor-product mass matrix applied row by row (14 instead of 28 instructions per element: -11 % VALU instructions,
    // 1.7-1.8 us per launch on the masked forms: box 56.6 -> 54.9, bits + box 57.7 -> 55.9 us, profiles/r2_ab2d_fmass.txt); not in the
    // generic mask / value-field form, whose register budget it would push from 4 to 3 waves per SIMD
    constexpr bool FMASS = HAS_F && ROWSTAGED;
    const float cx00 = p.T.q1mx[0], cx01 = p.T.q1mx[1], cx11 = p.T.q1mx[2], cy00 = p.T.q1my[0], cy01 = p.T.q1my[1], cy11 = p.T.q1my[2];
    const float alpha = p.T.alpha;
    // sum_g W_g f_g N_a(g) with f bilinear is (mass_x (x) mass_y) f.  x-stage, once per node row: g[n] = the row's forcing seen through
    // the thread's own elements (elements beyond the mesh excluded; the node shared with the right neighbour gets the rest over the
    // hand-over that o[] takes anyway, by linearity)
    auto fstage = [&](CfRow<E>& r) {
        if constexpr (FMASS) {
#pragma unroll
            for (int n = 0; n <= NW; ++n) r.g[n] = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (ex0 + e < p.nelx) {
                    r.g[e] = fmaf(cx01, r.f[e + 1], fmaf(cx00, r.f[e], r.g[e]));
                    r.g[e + 1] = fmaf(cx11, r.f[e + 1], cx01 * r.f[e]);
                }
            }
        }
    };

    // x-stage of the stiffness term, once per node row (after its Dirichlet select): du[], pn[] (q1cf_stage)
    auto sstage = [&](CfRow<E>& r) {
        if constexpr (ROWSTAGED) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if constexpr (HAS_NU) {
                    q1cf_stage(px0, px1, r.u[e], r.u[e + 1], r.n[e], r.n[e + 1], r.du[e], r.pn[e]);
                } else {              // nu == 1: its x-moment is the rule's
                    r.du[e] = r.u[e + 1] - r.u[e];
                    r.pn[e] = mx0;
                }
            }
        }
    };

    // one element layer between the lower row L (Dirichlet applied) and the freshly landed upper row U; cin holds the
    // contributions of the layer below to L's nodes, cout receives this layer's contributions to U's nodes
    // fresh: U has just landed from HBM (Dirichlet select and forcing x-stage still to do); not fresh: U came finished from the strip above
    auto layer = [&](auto fresh, int ey, const CfRow<E>& L, CfRow<E>& U, const float (&cin)[NW + 1], float (&cout)[NW + 1]) __attribute__((always_inline)) {
        const bool own_layer = ey >= e_from && ey <= e_until;
        const float cnt = (own_layer && col_owner) ? 1.f : 0.f;
        if constexpr (decltype(fresh)::value) { row_bc(U); fstage(U); }
        sstage(U);                        // (a row that came from the strip above through LDS restages here as well: nothing more is published)
        float o[NW + 1], le1 = 0.f, le2 = 0.f;
#pragma unroll
        for (int n = 0; n <= NW; ++n) { o[n] = cin[n]; cout[n] = 0.f; }
        if constexpr (FMASS) {            // y-stage of the forcing term for the whole row segment, and its energy  u . (M f)
#pragma unroll
            for (int n = 0; n <= NW; ++n) {
                const float tlo = fmaf(cy01, U.g[n], cy00 * L.g[n]), tup = fmaf(cy11, U.g[n], cy01 * L.g[n]);
                o[n] = fmaf(nb, tlo, o[n]);
                cout[n] = nb * tup;
                le2 = fmaf(U.u[n], tup, fmaf(L.u[n], tlo, le2));
            }
        }
        if constexpr (ROWSTAGED) {
            // per node: vertical difference of u and y-moment of nu (q1cf_elem)
            float V[NW + 1], S[NW + 1];
#pragma unroll
            for (int n = 0; n <= NW; ++n) {
                V[n] = U.u[n] - L.u[n];
                S[n] = HAS_NU ? fmaf(sy1, U.n[n], sy0 * L.n[n]) : my0;
            }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (ex0 + e < p.nelx) {       // elements beyond the domain are skipped (and: scheduling fence between elements)
                    const float a = STAGE_DU ? L.du[e] : L.u[e + 1] - L.u[e], b = STAGE_DU ? U.du[e] : U.u[e + 1] - U.u[e];
                    q1cf_elem(xm, ym, a, b, L.pn[e], U.pn[e], V[e], V[e + 1], S[e], S[e + 1], alpha, o[e], o[e + 1], cout[e], cout[e + 1], le1);
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (ex0 + e < p.nelx) {
                    const float U0 = L.u[e], UX = L.u[e + 1] - L.u[e], UY = U.u[e] - L.u[e], UXY = (U.u[e + 1] - U.u[e]) - UX;
                    float P = mx0, Q = 0.f, Pp = my0, Qp = 0.f;
                    if constexpr (HAS_NU) {
                        const float N0 = L.n[e], NX = L.n[e + 1] - N0, NY = U.n[e] - N0, NXY = (U.n[e + 1] - U.n[e]) - NX;
                        P = fmaf(mx1, NX, mx0 * N0);
                        Q = fmaf(mx1, NXY, mx0 * NY);
                        Pp = fmaf(my1, NY, my0 * N0);
                        Qp = fmaf(my1, NXY, my0 * NX);
                    }
                    const float A0 = fmaf(Q, my1, P * my0), A1 = fmaf(Q, my2, P * my1), A2 = fmaf(Q, my3, P * my2);
                    const float B0 = fmaf(Qp, mx1, Pp * mx0), B1 = fmaf(Qp, mx2, Pp * mx1), B2 = fmaf(Qp, mx3, Pp * mx2);
                    const float tX0 = fmaf(UXY, A1, UX * A0), tX1 = fmaf(UXY, A2, UX * A1);
                    const float tY0 = fmaf(UXY, B1, UY * B0), tY1 = fmaf(UXY, B2, UY * B1);
                    le1 += fmaf(h1, fmaf(UXY, tY1, UY * tY0), h0 * fmaf(UXY, tX1, UX * tX0));
                    float cU0 = 0.f, cUX = k0 * tX0, cUY = k1 * tY0, cUXY = fmaf(k0, tX1, k1 * tY1);
                    if constexpr (HAS_F) {
                        const float F0 = L.f[e], FX = L.f[e + 1] - F0, FY = U.f[e] - F0, FXY = (U.f[e + 1] - U.f[e]) - FX;
                        const float S0 = fmaf(mx1, FX, mx0 * F0), S1 = fmaf(mx1, FXY, mx0 * FY);
                        const float T0 = fmaf(mx2, FX, mx1 * F0), T1 = fmaf(mx2, FXY, mx1 * FY);
                        const float L0 = fmaf(my1, S1, my0 * S0), LX = fmaf(my1, T1, my0 * T0);
                        const float LY = fmaf(my2, S1, my1 * S0), LXY = fmaf(my2, T1, my1 * T0);
                        le2 += fmaf(LXY, UXY, fmaf(LY, UY, fmaf(LX, UX, L0 * U0)));
                        cU0 = nb * L0;
                        cUX = fmaf(nb, LX, cUX);
                        cUY = fmaf(nb, LY, cUY);
                        cUXY = fmaf(nb, LXY, cUXY);
                    }
                    const float g01 = cUX - cUXY, g10 = cUY - cUXY;
                    o[e] += (cU0 - cUX) - g10;
                    o[e + 1] += g01;
                    cout[e] += g10;
                    cout[e + 1] += cUXY;
                }
            }
        }
        e1_acc = fmaf(cnt, le1, e1_acc);
        e2_acc = fmaf(cnt, le2, e2_acc);
        if (W > 1 && chain_dn && ey == sb0) {
            // the strip's first row still lacks the contributions of the layer below it, which the strip below computes at its very end:
            // park this half in LDS (each thread re-reads its own words) and finish the row after the march
            const unsigned s0 = lds_addr(&cf_seam[W > 1 ? sub - 1 : 0][0][tid]);
#pragma unroll
            for (int n = 0; n <= NW; ++n) lds_st(s0 + (4 * NW + 4 + n) * CF_TS * 4, o[n]);
#pragma unroll
            for (int n = 0; n < NW; ++n) lds_st(s0 + (5 * NW + 5 + n) * CF_TS * 4, L.keep[n]);
        } else {
            emit_row(o, L.keep, ey, ey >= r_from, L.keepx);
        }
    };
    // chained strips: row / carry hand-over with the neighbouring strip of the workgroup.  Thread t of one strip talks to thread t of the
    // other, which sits in the wave of the same number: one flag per wave and direction
    auto publish_row = [&](const CfRow<E>& r) {
        const unsigned s0 = lds_addr(&cf_seam[W > 1 ? sub - 1 : 0][0][tid]);
#pragma unroll
        for (int n = 0; n <= NW; ++n) {
            lds_st(s0 + n * CF_TS * 4, r.u[n]);
            if constexpr (HAS_NU) lds_st(s0 + (NW + 1 + n) * CF_TS * 4, r.n[n]);
            if constexpr (FMASS) lds_st(s0 + (2 * NW + 2 + n) * CF_TS * 4, r.g[n]);
            else if constexpr (HAS_F) lds_st(s0 + (2 * NW + 2 + n) * CF_TS * 4, r.f[n]);
        }
        if (lane == 0) lds_st(lds_addr(&cf_sflag[W > 1 ? sub - 1 : 0][0][wv]), 1u);
    };
    auto fetch_row = [&](CfRow<E>& r) {
        spin_until(&cf_sflag[sub][0][wv], 1u);
        const unsigned s0 = lds_addr(&cf_seam[sub][0][tid]);
#pragma unroll
        for (int n = 0; n <= NW; ++n) lds_ld_nowait(r.u[n], s0 + n * CF_TS * 4);
        lds_wait(r.u);
        if constexpr (HAS_NU) {
#pragma unroll
            for (int n = 0; n <= NW; ++n) lds_ld_nowait(r.n[n], s0 + (NW + 1 + n) * CF_TS * 4);
            lds_wait(r.n);
        }
        if constexpr (FMASS) {
#pragma unroll
            for (int n = 0; n <= NW; ++n) lds_ld_nowait(r.g[n], s0 + (2 * NW + 2 + n) * CF_TS * 4);
            lds_wait(r.g);
        } else if constexpr (HAS_F) {
#pragma unroll
            for (int n = 0; n <= NW; ++n) lds_ld_nowait(r.f[n], s0 + (2 * NW + 2 + n) * CF_TS * 4);
            lds_wait(r.f);
        }
    };
    auto publish_carry = [&](const float (&c)[NW + 1]) {
        const unsigned s0 = lds_addr(&cf_seam[sub][0][tid]);
#pragma unroll
        for (int n = 0; n <= NW; ++n) lds_st(s0 + (3 * NW + 3 + n) * CF_TS * 4, c[n]);
        if (lane == 0) lds_st(lds_addr(&cf_sflag[sub][1][wv]), 1u);
    };

    auto set_prio = [&](int e) {
        switch (((ey_end - e) >> 1) & 3) {          // progress-dependent wave priority (profiles/README.md)
            case 0: __builtin_amdgcn_s_setprio(0); break;
            case 1: __builtin_amdgcn_s_setprio(1); break;
            case 2: __builtin_amdgcn_s_setprio(2); break;
            default: __builtin_amdgcn_s_setprio(3); break;
        }
    };

    constexpr std::true_type FRESH{};
    constexpr std::false_type LANDED{};
    if (active) {                     // (a workgroup's unused sub-strips only join the final reduction)
    CfRow<E> RA, RB;
    float carryA[NW + 1], carryB[NW + 1];
#pragma unroll
    for (int n = 0; n <= NW; ++n) carryA[n] = carryB[n] = 0.f;
    constexpr std::true_type NT_U{};
    constexpr std::false_type PLAIN_U{};
    row_issue(PLAIN_U, ey_begin, RA);
    row_bc(RA);
    fstage(RA);
    sstage(RA);
    if constexpr (W > 1) {
        if (chain_dn) publish_row(RA);
    }
    int ey = ey_begin;
    bool odd = false;
    const int n_main = chain_up ? ey_end - 1 : ey_end;         // chain_up: the strip's last layer takes its upper row from the strip above (LDS)
    auto trip2 = [&](auto nt_u) __attribute__((always_inline)) {
        set_prio(ey);
        row_issue(nt_u, ey + 1, RB);
        layer(FRESH, ey, RA, RB, carryA, carryB);
        row_issue(nt_u, ey + 2, RA);
        layer(FRESH, ey + 1, RB, RA, carryB, carryA);
        ey += 2;
    };
    if constexpr (XCH) {
        // the rows a neighbouring strip reads as well (the strip's first two and last two) with plain loads, the rows it owns alone
        // non-temporal: the first and the last two-row trip peeled out of the loop, no branch inside it
        if (ey + 1 < n_main) trip2(PLAIN_U);
        while (ey + 3 < n_main) trip2(NT_U);
        if (ey + 1 < n_main) trip2(PLAIN_U);
    } else {                          // (the loop as every other form has always had it: through trip2 the two-element forms compile to a few instructions more)
        for (; ey + 1 < n_main; ey += 2) {
            set_prio(ey);
            row_issue(PLAIN_U, ey + 1, RB);
            layer(FRESH, ey, RA, RB, carryA, carryB);
            row_issue(PLAIN_U, ey + 2, RA);
            layer(FRESH, ey + 1, RB, RA, carryB, carryA);
        }
    }
    if (ey < n_main) {
        set_prio(ey);
        row_issue(PLAIN_U, ey + 1, RB);
        layer(FRESH, ey, RA, RB, carryA, carryB);
        odd = true;
        ++ey;
    }
    if constexpr (W > 1) {
        if (chain_up) {               // ey == ey_end - 1
            __builtin_amdgcn_s_setprio(0);
            if (odd) { fetch_row(RA); layer(LANDED, ey, RB, RA, carryB, carryA); publish_carry(carryA); }
            else { fetch_row(RB); layer(LANDED, ey, RA, RB, carryA, carryB); publish_carry(carryB); }
        }
    }
    if (top_row) {                // the last row of the domain: only the layer below it contributes
        float o[NW + 1], keep[NW];
#pragma unroll
        for (int n = 0; n <= NW; ++n) o[n] = odd ? carryB[n] : carryA[n];
#pragma unroll
        for (int n = 0; n < NW; ++n) keep[n] = odd ? RB.keep[n] : RA.keep[n];
        emit_row(o, keep, p.ny - 1, true, odd ? RB.keepx : RA.keepx);
        flush_store();
    }
    if constexpr (W > 1) {
        if (chain_dn) {               // finish the strip's first row: parked half + the carry of the strip below
            spin_until(&cf_sflag[sub - 1][1][wv], 1u);
            const unsigned s0 = lds_addr(&cf_seam[sub - 1][0][tid]);
            float o[NW + 1], cy[NW + 1], keep[NW];
#pragma unroll
            for (int n = 0; n <= NW; ++n) lds_ld_nowait(o[n], s0 + (4 * NW + 4 + n) * CF_TS * 4);
            lds_wait(o);
#pragma unroll
            for (int n = 0; n <= NW; ++n) lds_ld_nowait(cy[n], s0 + (3 * NW + 3 + n) * CF_TS * 4);
            lds_wait(cy);
#pragma unroll
            for (int n = 0; n < NW; ++n) lds_ld_nowait(keep[n], s0 + (5 * NW + 5 + n) * CF_TS * 4);
            lds_wait(keep);
#pragma unroll
            for (int n = 0; n <= NW; ++n) o[n] += cy[n];
            emit_row(o, keep, sb0, true);
            flush_store();
        }
    }
    }                                 // active

    if constexpr (W > 1) {            // a hand-over poll that ran into its bound: NaN sums + the sticky error word (never silent)
        e1_acc += spin_poison;
        sq_acc += spin_poison;
        if (spin_poison != spin_poison && p.counter != nullptr && (threadIdx.x & 63u) == 0u) atomicOr(p.counter + DN_WS_ERRWORD, 1u);
    }
    if (p.want_sums) finish_sums(p, e1_acc, e2_acc, sq_acc, (int)threadIdx.x, (int)blockDim.x, red, &last_flag);
}

template <int E, bool VEC, int FL>
static void cf_launch_one(const PoissonParams& pp, const Geom2D& g, int batch, hipStream_t s) {
    if constexpr (E == 4 && VEC && (FL & CF_UA) == 0) {
        if (g.W == CF_W) {            // chained sub-strips (plan2d): W strips per workgroup
            hipLaunchKernelGGL((poisson2d_q1_cf_kernel<E, VEC, FL, CF_W>), dim3(g.chunks, (g.strips + CF_W - 1) / CF_W, batch),
                               dim3(CF_TS * CF_W), 0, s, pp);
            return;
        }
    }
    hipLaunchKernelGGL((poisson2d_q1_cf_kernel<E, VEC, FL, 1>), dim3(g.chunks, g.strips, batch), dim3(g.T), 0, s, pp);
}

template <int E, bool VEC, int UAF = 0>
static void cf_launch_flags(const PoissonParams& pp, const Geom2D& g, int batch, hipStream_t s) {
    const bool any = pp.bc[0].kind >= 0 || pp.bc[1].kind >= 0;
    bool u8c = any, packed = false;
    for (int k = 0; k < 2; ++k) {
        if (pp.bc[k].kind >= 0 && (!pp.bc[k].mask_is_u8 || pp.bc[k].field)) u8c = false;
        if (pp.bc[k].kind == DN_MASK_BITS || pp.bc[k].kind == DN_MASK_BOX) packed = true;     // dn_poisson_apply admits no mix with mask images
    }
    const int nbits = (pp.bc[0].kind == DN_MASK_BITS) + (pp.bc[1].kind == DN_MASK_BITS);
    const bool one = (pp.bc[0].kind >= 0) != (pp.bc[1].kind >= 0);        // one condition: the instantiations without the absent one's selects
    const int nf = (pp.nu ? CF_NU : 0) | (pp.f ? CF_F : 0);
#define DN_CF(FLAGS)                                                                         \
    (!any ? cf_launch_one<E, VEC, (FLAGS) | UAF>(pp, g, batch, s)                                  \
          : packed ? (nbits == 2 ? cf_launch_one<E, VEC, (FLAGS) | UAF | CF_BC_PACKED | CF_PK_NB2>(pp, g, batch, s)          \
                     : nbits == 1 ? (one ? cf_launch_one<E, VEC, (FLAGS) | UAF | CF_BC_PACKED | CF_PK_NB1 | CF_ONE>(pp, g, batch, s)        \
                                         : cf_launch_one<E, VEC, (FLAGS) | UAF | CF_BC_PACKED | CF_PK_NB1>(pp, g, batch, s))        \
                     : one ? cf_launch_one<E, VEC, (FLAGS) | UAF | CF_BC_PACKED | CF_ONE>(pp, g, batch, s)                   \
                           : cf_launch_one<E, VEC, (FLAGS) | UAF | CF_BC_PACKED>(pp, g, batch, s))                   \
          : u8c ? (one ? cf_launch_one<E, VEC, (FLAGS) | UAF | CF_BC_U8C | CF_ONE>(pp, g, batch, s)                \
                       : cf_launch_one<E, VEC, (FLAGS) | UAF | CF_BC_U8C>(pp, g, batch, s))                \
                : cf_launch_one<E, VEC, (FLAGS) | UAF | CF_BC>(pp, g, batch, s))
    switch (nf) {
        case 0: DN_CF(0); break;
        case CF_NU: DN_CF(CF_NU); break;
        case CF_F: DN_CF(CF_F); break;
        default: DN_CF(CF_NU | CF_F); break;
    }
#undef DN_CF
}

int poisson2d_q1_cf_chain() { return CF_W; }       // what plan2d may put into Geom2D::W

int launch_poisson2d_q1_cf(const PoissonParams& pp, const Geom2D& g, int batch, bool vec, hipStream_t s) {
    if (g.W > 1 && !(g.W == poisson2d_q1_cf_chain() && g.E == 4 && vec && g.T == CF_TS && g.R + 3 <= CF_NSLOT)) return DN_E_BADARG;
    if (g.ua) {                   // rows of 4 k + 1 nodes (plan2d): the vector kernel on 4-byte aligned rows, last node column in the last thread column
        if (g.E != 4 || g.W != 1 || (pp.nx & 3) != 1 || pp.nx < 9) return DN_E_BADARG;
        cf_launch_flags<4, true, CF_UA>(pp, g, batch, s);
        return 0;
    }
    if (g.E == 4 && vec) { cf_launch_flags<4, true>(pp, g, batch, s); return 0; }
    if (g.E == 2 && vec) { cf_launch_flags<2, true>(pp, g, batch, s); return 0; }
    if (g.E == 2) { cf_launch_flags<2, false>(pp, g, batch, s); return 0; }
    return DN_E_UNSUPPORTED;
}

}  // namespace dn
