// The march of one thread of the element-march kernels (strongform.hip, fosls.hip, helmholtz.hip, eikonal.hip), written once: the BODY of a
// kernel, included between its braces with the template parameters P, NGP, FK (forcing: constant / nodal / at the Gauss points), MASK
// and BCF (any condition / any value field), the type `Op` and the parameters `p` in scope.  It is text and not a function on purpose:
// with the body in an inlined function that receives p, the compiler splits the kernel's copy of the parameters into registers at entry
// (every member loaded up front, those of the reduction tail included): 6 to 8 more SGPRs in every kernel and an occupancy step lost
// in several; as a function with only the loop over the conditions' base pointers left in the kernel, 4 of the 36 degree-1 strong-form
// kernels still lose a step (profiles/elem2d_refactor.txt, section 1, variants b and c).
//
// grid = (chunks_x, strips_y, B), block = T threads; one element column per thread (chunks overlap by one thread column).  The P new
// node rows of layer k + 1 (and its Gauss-point forcing) are requested before the arithmetic of layer k; the finished rows of layer k
// are stored after that request (fsdt.hip has the reasons).  The operator is an object of type Op that lives in the thread's registers:
//   NF (output fields), NS (running sums, 1 or 2), FOLDS_OK (see element)
//   Raw                          its nodal arrays of one raw row (the conditioned field u among them)
//   init(p, b, nps)              per-sample base pointers; sets `ub`, the base of u (absent inputs alias it)
//   start(p)                     its scale and the start values of its nodal arrays
//   out_base(p, k, b, nps)       sample b of output field k, or nullptr
//   issue(p, rowoff, x0, w, issue_f)   requests its raw row, and the nodal forcing (issue_f()) at its place in the order
//   raw_u(w, n), put(p, w, r, n, v)   a landed row into slot r: v is u after the two conditions
//   fixed_row(r, bits)           optional (elem2d_has_fixed_row): after put() of a whole row into slot r, its Dirichlet nodes as bits
//   shift(n)                     slot P becomes slot 0
//   element(p, fn, fg, okf, g)   adds the element's contributions to g; returns its share of sum 0.  FOLDS_OK: it weighs them with okf
//                                itself (g is acc); otherwise the march adds okf * g to acc afterwards.  The two round differently
//   finish_row(p, k, row, fixed, x0)  a complete node row of field k before it is parked; returns its share of sum 1
//   write_sums(p, tot)           the launch's totals
constexpr int NF = Op::NF, NS = Op::NS;
constexpr int NB = P + 1;
constexpr int NW = P;                  // nodes owned per thread per node row
constexpr int G = NGP * NGP;
static_assert(MASK || !BCF, "a value field belongs to a condition");
static_assert(NS == 1 || NS == 2, "one or two running sums");
const int T = (int)blockDim.x, tid = (int)threadIdx.x;
const int chunk = blockIdx.x, b = blockIdx.z;
const int R = p.rows_per_strip;
const int ey_own = (int)blockIdx.y * R;
const int q = chunk * (T - 1) + tid;
const int ex0 = q, x0 = ex0 * P;
const bool col_owner = !(chunk > 0 && tid == 0);
const int64_t nps = (int64_t)p.nx * p.ny;
const int nel = p.nelx * p.nely;
const int ey_begin = ey_own > 0 ? ey_own - 1 : ey_own;        // the layer under the strip's first node row is recomputed
const int ey_end = min(ey_own + R, p.nely);
const int ymax = p.ny - 1;
const bool has_elem = ex0 < p.nelx;
const float okf = has_elem ? 1.f : 0.f;      // threads right of the mesh compute on clamped data, scaled by 0
const unsigned exc = (unsigned)min(ex0, p.nelx - 1);

Op op;
op.init(p, b, nps);
const float* ub = op.ub;
const float* fb = FK == 1 ? p.f + (p.f_batched ? (int64_t)b * nps : 0) : ub;
const float* fgb = FK == 2 ? p.fgp + (p.f_batched ? (int64_t)b * G * nel : 0) : ub;
float* ob[NF];
#pragma unroll
for (int k = 0; k < NF; ++k) ob[k] = op.out_base(p, k, b, nps);
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
op.start(p);

__shared__ float xch[2][P * NF][256];        // [parity][node row of the layer, field][thread]
__shared__ double red[16];
__shared__ int last_flag;

float fn[NB][NB], acc[NF][NB][NB];
unsigned fixed[NB];
#pragma unroll
for (int r = 0; r < NB; ++r) {
    fixed[r] = 0u;
#pragma unroll
    for (int n = 0; n < NB; ++n) {
        fn[r][n] = 0.f;
#pragma unroll
        for (int k = 0; k < NF; ++k) acc[k][r][n] = 0.f;
    }
}

struct RawRow {
    typename Op::Raw o;
    float f[FK == 1 ? NW + 1 : 1];
    float mf[MASK ? 2 : 1][NW + 1], bf[BCF ? 2 : 1][NW + 1];
    uint8_t mb[MASK ? 2 : 1][NW + 1];
};
auto row_issue = [&](int yr, RawRow& w) {
    const unsigned rowoff = (unsigned)min(yr, ymax) * (unsigned)p.nx;
    op.issue(p, rowoff, x0, w.o, [&] {          // the operator places the request of the nodal forcing among its own
        if constexpr (FK == 1) load_seg<NW, false>(fb, rowoff, x0, p.nx, w.f);
    });
    if constexpr (MASK) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (p.mask_kind[k] == 2) load_seg<NW, false>(mfp[k], rowoff, x0, p.nx, w.mf[k]);
            else if (p.mask_kind[k] == 1) load_seg<NW, false>(mbp[k], rowoff, x0, p.nx, w.mb[k]);
        }
    }
    if constexpr (BCF) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (p.bcf[k]) load_seg<NW, false>(bcfb[k], rowoff, x0, p.nx, w.bf[k]);
    }
};
// landed row -> slot r: the two Dirichlet substitutions of u in order (condition 2 wins where both hold)
auto row_consume = [&](const RawRow& w, int r) {
    unsigned bits = 0u;
#pragma unroll
    for (int n = 0; n <= NW; ++n) {
        float v = op.raw_u(w.o, n);
        if constexpr (MASK) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const bool fx = p.mask_kind[k] == 2 ? (w.mf[k][n] > 0.5f) : (p.mask_kind[k] == 1 ? (w.mb[k][n] != 0) : false);
                float bv = p.bcv[k];
                if constexpr (BCF) bv = p.bcf[k] ? w.bf[k][n] : bv;
                v = fx ? bv : v;
                bits |= fx ? (1u << n) : 0u;
            }
        }
        op.put(p, w.o, r, n, v);
        if constexpr (FK == 1) fn[r][n] = w.f[n];
    }
    fixed[r] = bits;
    if constexpr (elem2d_has_fixed_row<Op>::value) op.fixed_row(r, bits);
};
auto fg_issue = [&](int ey, float (&w)[G]) {
    if constexpr (FK == 2) {
        const unsigned eoff = (unsigned)min(ey, p.nely - 1) * (unsigned)p.nelx + exc;
#pragma unroll
        for (int gq = 0; gq < G; ++gq) w[gq] = ld_at<float>(fgb, eoff + (unsigned)(gq * nel));
    }
};

double sums[NS];
#pragma unroll
for (int k = 0; k < NS; ++k) sums[k] = 0.0;
int par = 0;

// finished node rows wait here until flush_rows() stores them
float pend[P][NF][NW];
unsigned pend_off[P];
bool pend_st[P];
#pragma unroll
for (int r = 0; r < P; ++r) pend_st[r] = false;
auto flush_rows = [&]() {
#pragma unroll
    for (int r = 0; r < P; ++r) {
        if (pend_st[r]) {
#pragma unroll
            for (int k = 0; k < NF; ++k)
                if (NF == 1 || ob[k]) store_seg<NW, false>(ob[k], pend_off[r], x0, p.nx, pend[r][k]);
        }
        pend_st[r] = false;
    }
};
// Emit node row yr from acc[.][r] (+ the left neighbour's hand-over for n == 0): the row is complete here
auto emit_row = [&](int r, int slot, int yr, bool owned_row) {
    float (*const xc)[256] = &xch[par][r % P * NF];      // the row's slot, addressed once for the stores and the loads
#pragma unroll
    for (int k = 0; k < NF; ++k) xc[k][tid] = acc[k][r][NW];
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS-only barrier (loads stay in flight)
    const bool mine = owned_row && col_owner;
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        const float left = (tid > 0) ? xc[k][tid - 1] : 0.f;
#pragma unroll
        for (int n = 0; n < NW; ++n) pend[slot][k][n] = acc[k][r][n] + (n == 0 ? left : 0.f);
        const float rs = op.finish_row(p, k, pend[slot][k], fixed[r], x0);
        if constexpr (NS == 2) sums[1] += mine ? (double)rs : 0.0;
    }
    pend_off[slot] = (unsigned)yr * (unsigned)p.nx;
    pend_st[slot] = mine && (NF > 1 || ob[0] != nullptr);      // one field: the test of its pointer here, not at every store
};

{
    RawRow W[P];
    float fgw[FK == 2 ? G : 1], fgc[G];
#pragma unroll
    for (int gq = 0; gq < G; ++gq) fgc[gq] = 0.f;
    {
        RawRow w0;
        row_issue(ey_begin * P, w0);
#pragma unroll
        for (int r = 1; r <= P; ++r) row_issue(ey_begin * P + r, W[r - 1]);       // all P + 1 rows of the first layer in flight together
        if constexpr (FK == 2) fg_issue(ey_begin, fgw);
        row_consume(w0, 0);
    }
    for (int ey = ey_begin; ey < ey_end; ++ey) {
#pragma unroll
        for (int r = 1; r <= P; ++r) row_consume(W[r - 1], r);
        if constexpr (FK == 2) {
#pragma unroll
            for (int gq = 0; gq < G; ++gq) fgc[gq] = fgw[gq];
        }
#pragma unroll
        for (int r = 1; r <= P; ++r) row_issue((ey + 1) * P + r, W[r - 1]);      // rows beyond the mesh re-read the last one (unused)
        if constexpr (FK == 2) fg_issue(ey + 1, fgw);
        flush_rows();
        const bool own_layer = ey >= ey_own;
        float gl[NF][NB][NB];
        float (&g)[NF][NB][NB] = Op::FOLDS_OK ? acc : gl;     // an element that weighs its contributions itself adds straight into acc
        if constexpr (!Op::FOLDS_OK) {
#pragma unroll
            for (int k = 0; k < NF; ++k)
#pragma unroll
                for (int jb = 0; jb < NB; ++jb)
#pragma unroll
                    for (int ib = 0; ib < NB; ++ib) gl[k][jb][ib] = 0.f;
        }
        const float es = op.element(p, fn, fgc, okf, g);
        sums[0] += (own_layer && col_owner && has_elem) ? (double)es : 0.0;      // every element once: its owner thread, its own strip
        if constexpr (!Op::FOLDS_OK) {
#pragma unroll
            for (int k = 0; k < NF; ++k)
#pragma unroll
                for (int jb = 0; jb < NB; ++jb)
#pragma unroll
                    for (int ib = 0; ib < NB; ++ib) acc[k][jb][ib] = fmaf(okf, gl[k][jb][ib], acc[k][jb][ib]);
        }
#pragma unroll
        for (int r = 0; r < P; ++r) emit_row(r, r, ey * P + r, own_layer);
        par ^= 1;
#pragma unroll
        for (int n = 0; n <= NW; ++n) {
            op.shift(n);
            fn[0][n] = fn[P][n];
#pragma unroll
            for (int k = 0; k < NF; ++k) {
                acc[k][0][n] = acc[k][P][n];
#pragma unroll
                for (int r = 1; r <= P; ++r) acc[k][r][n] = 0.f;
            }
        }
        fixed[0] = fixed[P];
    }
    flush_rows();
    if (ey_end == p.nely) {
        emit_row(0, 0, p.ny - 1, true);
        flush_rows();
    }
}

// per element / node row in fp32, per thread in fp64, then the fixed-order fp64 reduction of dn_reduce.h
if (p.want_sums) {
    const int nthreads = (int)blockDim.x;
    double* parts[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) parts[k] = p.part + k * launch_workgroups();
    elem2d_block_sums(sums, red, tid, nthreads);
    double tot[NS];
    if (last_arriver_sums<NS, 8, false, true>(parts, p.counter, sums, tid, nthreads, &last_flag, tot)) {
        elem2d_block_sums(tot, red, tid, nthreads);
        if (tid == 0) {
            op.write_sums(p, tot);
            arrival_reset(p.counter);
            p.counter[DN_WS_TICKET_WORD] = 0u;
        }
    }
}
