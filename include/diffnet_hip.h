/*
 * diffnet_hip.h -- C ABI of libdiffnet_hip.so, the MI355X (gfx950) implementation of the
 * DiffNet FEM Gauss-quadrature hot path.
 *
 * Plain pointers and sizes only: no torch types cross this boundary.  Every pointer is a
 * DEVICE pointer (HBM resident) unless stated otherwise; tensors are contiguous fp32 in the
 * reference's layouts: nodal fields (B,1,Ny,Nx) / (B,1,Nz,Ny,Nx), Gauss-point fields
 * (B,G,nelY,nelX) / (B,G,nelZ,nelY,nelX) with G = ngp_1d^nsd and the Gauss-point id
 * g = (kg*ngp + jg)*ngp + ig (x fastest), local basis id a = (kb*nbf + jb)*nbf + ib.
 * `stream` is a hipStream_t passed as void* (NULL = default stream).  All entry points are
 * asynchronous on `stream`, allocate nothing, never synchronise, and are graph-capturable.
 * Return value: 0 on success, a positive hipError_t from the launch, or a negative DN_E_* code
 * for an argument the kernels do not support (nothing is launched in that case).
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * reference repository root).
 */
#ifndef DIFFNET_HIP_H
#define DIFFNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DN_ABI_VERSION 10

#define DN_E_BADARG (-1)    /* null pointer / non-positive size / unsupported combination   */
#define DN_E_UNSUPPORTED (-2) /* (nsd, degree, ngp) outside the compiled instantiations      */
#define DN_E_WORKSPACE (-3)  /* workspace too small                                           */
#define DN_E_HANDOVER (-4)   /* dn_workspace_status: a launch that used the workspace ran a bounded LDS hand-over poll to its
                                limit (chained-strip plans of dn_poisson_apply / dn_fsdt_apply); its results are NaN        */

/* Process-wide tuning / A-B switches (launch geometry overrides, kernel-variant selection).  They are NOT part of the
 * numerical contract: every setting yields the same results to rounding.  The table is initialised ONCE when the library
 * is loaded, from the environment variables DN_<KEY>; afterwards the environment is never read again (no getenv on the
 * launch path) and the only way to change a switch is this call.  Keys (the table kKeys in csrc/dn_api.hip):
 *   "PLAN2D" ("T,E,R[,W]": threads per strip, elements per thread, node rows per strip, W >= 2 = chain strips per workgroup
 *   where the closed-form Q1 kernel can), "PLAN3D" ("TX,TY,E,R"; E = 1 is ignored by launches only the two-element form serves: box faces,
 *   fold_prev, f_is_load), "PLAN_FSDT" ("T,R"),
 *   "Q1_RULE_KERNEL" (non-empty: per-Gauss-point 2-D Q1 kernels instead of the closed form),
 *   "GPE_GATHER" (non-empty: per-node gather adjoint of gauss_pt_eval), "GPE_TILED" (non-empty: tiled LDS adjoint instead of the
 *   marching 3-D Q1 adjoint), "Q1_3D_T16" (non-empty: the 3-D Q1 kernel form in which every thread loads its own nodes),
 *   "Q1_3D_E1SUM" (non-empty: 3-D stiffness energy summed Gauss point by Gauss point), "Q1_3D_E1" (non-empty: the 3-D node-owner kernel with one element per thread also where the two-element form applies),
 *   "FSDT_GENERIC" (non-empty: the table-driven
 *   FSDT element also for Q2 with the symmetric 3-point rule, whose middle point otherwise runs a specialised form),
 *   "PLAN_FSDT" also takes "64,R,W": W one-wave sub-strips chained per workgroup,
 *   "HANDOVER_SPIN_LIMIT" (integer: bound of the chained plans' LDS hand-over polls instead of the built-in 2^20 -- a test hook for the
 *   error path of dn_workspace_status; a small value makes healthy launches fail), "CONV2D_V1" (non-empty: the round-2 im2col forms of
 *   dn_conv2d_k4s2_down / _up / _wrw also where the raw-row-tile forms of round 4 apply), "CONV_WRW_WGS" (integer: workgroups a
 *   dn_conv2d_k4s2_wrw launch aims at when it splits K; default 1024), "Q1_3D_N2" (non-empty: the round-3 per-Gauss-point form of the 3-D Q1
 *   two-element kernel also where the closed-form-in-z kernel of round 4, csrc/poisson3d_q1_cf.hip, applies),
 *   "FSDT_FORM" ("elem": dn_fsdt_apply runs the element form of rounds 1-3, csrc/fsdt.hip, instead of the assembled-stencil form of round 4,
 *   csrc/fsdt_st.hip, which is the default for Q1 and Q2 meshes; "stencil": the stencil form also for Q3 meshes, where the element form is the default).
 *   dn_poisson_coef_grad takes the node rows per strip of its 2-D launch from the R of "PLAN2D" (its results do not depend on it).
 *   Beside these, the table keeps the switches of the HOST layer (kHostKeys in csrc/dn_api.hip), which no kernel or entry point reads:
 *   "COEF_GRAD" ("composed": diffnet_amd.ops differentiates the Poisson losses with respect to nu / f on the composed operators, as
 *   before dn_poisson_coef_grad existed, instead of with that launch).  value NULL or "" clears the switch.
 * Returns 0, or DN_E_BADARG for an unknown key / over-long value.  Not thread-safe against concurrent launches.
 * No reference counterpart (the reference has no tuning surface). */
int dn_config_set(const char *key, const char *value);
/* Current value of a switch ("" when unset), NULL for an unknown key. */
const char *dn_config_get(const char *key);

/* Geometry + 1-D reference-element tables of one structured mesh.
 * Mirrors what DiffNetFEM.__init__ derives (DiffNet/DiffNetFEM.py:25-126):
 *   basis[ig][ib]  = phi_ib(xi_ig)          1-D Lagrange basis at the 1-D Gauss points
 *   dbasis[ig][ib] = phi'_ib(xi_ig)         derivative in reference coordinates
 *   gpw[ig]        1-D Gauss weights,  scale[d] = 2/h_d  (d = x,y,z)
 * The nd tables of the reference (N_gp, dN_x_gp, ...) are the tensor products of these; the
 * fused kernels apply them axis by axis (sum factorisation) instead of materialising them. */
typedef struct dn_mesh {
    int32_t nsd;          /* 2 or 3                                                     */
    int32_t degree;       /* fem_basis_deg: 1, 2 or 3                                   */
    int32_t ngp;          /* ngp_1d: 1..4                                               */
    int32_t batch;        /* B                                                          */
    int32_t nx, ny, nz;   /* nodes per axis (nz = 1 when nsd == 2)                      */
    float scale[3];       /* 2/hx, 2/hy, 2/hz                                           */
    float gpw[4];
    float basis[4][4];
    float dbasis[4][4];
} dn_mesh;

/* One Dirichlet condition: u <- where(mask > 0.5, value, u) with value = field[node] when
 * `field` is non-null (broadcast over the batch when field_batched == 0) else the constant.
 * Mirrors the torch.where lines of the loss bodies, e.g. IBN/poisson-2d/parametric/IBN_2D.py:119-121,
 * examples/poisson/single_instance/e8_2d_poisson_mms.py:120.
 * Mask formats (`mask_kind`):
 *   DN_MASK_F32  the reference's fp32 image, compared with 0.5            (4 B per node)
 *   DN_MASK_U8   uint8 / bool, non-zero = set                             (1 B per node)
 *   DN_MASK_BITS one bit per node: node x of a node row is bit (x & 31) of 32-bit word (x >> 5) of that row, rows
 *                `row_words` words apart (>= ceil(nx / 32)), rows of a sample contiguous, samples ny*[nz*]row_words words
 *                apart -- what dn_pack_mask_bits() writes                 (1/8 B per node)
 *   DN_MASK_BOX  no array at all: the condition holds on the domain faces named in `box_faces` (IBN_2D.py:69-73 builds exactly
 *                this mask as an image, DiffNet/datasets/single_instances/rectangles.py:16,232-233 likewise); `mask` is ignored
 * BITS and BOX take a constant `value` (field must be NULL) and are implemented by the 2-D Q1 kernels with nodal / absent
 * forcing (the IBN_2D / bench path); every other kernel returns DN_E_UNSUPPORTED for them -- expand with dn_unpack_mask_bits(). */
enum { DN_MASK_F32 = 0, DN_MASK_U8 = 1, DN_MASK_BITS = 2, DN_MASK_BOX = 3 };
enum { DN_FACE_XLO = 1, DN_FACE_XHI = 2, DN_FACE_YLO = 4, DN_FACE_YHI = 8, DN_FACE_ZLO = 16, DN_FACE_ZHI = 32 };
typedef struct dn_dirichlet {
    const void *mask;     /* (B,1,*N) or (1,1,*N); NULL = condition absent (DN_MASK_BOX: ignored) */
    const float *field;   /* optional Dirichlet values                                  */
    float value;
    int32_t mask_kind;    /* DN_MASK_*  (0 / 1 keep their round-1 meaning "mask_is_u8") */
    int32_t mask_batched; /* 1: (B,...), 0: one mask shared by the whole batch          */
    int32_t field_batched;
    int32_t box_faces;    /* DN_MASK_BOX: bit set of DN_FACE_*                          */
    int32_t row_words;    /* DN_MASK_BITS: 32-bit words per node row                    */
} dn_dirichlet;

/* uint8 / fp32 mask image -> DN_MASK_BITS layout and back (one launch each; rows = B*ny[*nz] node rows of nx nodes).
 * The reference keeps masks as fp32 images in its datasets (DiffNet/datasets/parametric/images.py:30); packing them once when
 * the dataset is placed in HBM turns a 4 (or 1) B/node stream of the loss into 1/8 B/node. */
int dn_pack_mask_bits(const void *mask, int32_t mask_kind, int64_t rows, int32_t nx, int32_t row_words, uint32_t *bits, void *stream);
int dn_unpack_mask_bits(const uint32_t *bits, int64_t rows, int32_t nx, int32_t row_words, uint8_t *mask_u8, void *stream);

/* Arguments of the fused Poisson operator
 *     out_a = zero_on_dirichlet( sum_e sum_g W_g ( alpha * nu_g * gradN_a . grad u_g  -  beta * N_a * f_g ) )
 *     energy = sum_{b,e,g} W_g ( c * nu_g * |grad u_g|^2 - u_g * f_g ),      W_g = gpw_g * wscale
 * evaluated in ONE pass over the nodal fields with element->node assembly in gather form
 * (deterministic, no atomics).  It replaces, per call:
 *   - energy loss + its gradient  (alpha = 2c, beta = 1):  IBN_2D.py:116-134, IBN_3D.py:114-136,
 *     solve_in_object_3d.py:75-102, 12_klsum.py:53-78, e8_2d_poisson_mms.py:152-180 -- i.e. 5-6
 *     gauss_pt_eval calls (DiffNet/DiffNetFEM.py:7-18) + ~8 elementwise ops + autograd backward;
 *   - weak-form residual + Q1_*_vector_assembly + BC mask + sum(R^2) (alpha = beta = 1):
 *     12_klsum.py:80-132, e8_2d_poisson_mms.py:92-150, e8_3d_poisson_mms.py:89-139, tests/test.py:43-79;
 *   - the backward of the residual loss: the operator is symmetric, so grad_u = apply(v = 2R, f absent). */
typedef struct dn_poisson_args {
    const float *u;        /* (B,1,*N) nodal field                                      */
    const float *nu;       /* (B,1,*N) or NULL (nu == 1)                                */
    const float *f;        /* (B,1,*N) nodal forcing or NULL                            */
    const float *f_gp;     /* (Bf,G,*nel) forcing at Gauss points or NULL (exclusive with f) */
    int32_t nu_batched;    /* 0: one (1,1,*N) field for the whole batch                 */
    int32_t f_batched;     /* same for f / f_gp                                         */
    dn_dirichlet bc[2];    /* applied in order                                          */
    float alpha, beta, c, wscale;
    float out_scale;       /* out is multiplied by this (e.g. 1/(B*nel) of torch.mean)  */
    float *out;            /* (B,1,*N) or NULL                                          */
    double *energy;        /* device scalar: sum (unscaled) or NULL                     */
    double *sumsq;         /* device scalar: sum over nodes of (out/out_scale)^2 or NULL */
    void *workspace;       /* dn_poisson_workspace_bytes() bytes, needed when energy or sumsq is set. Must be
                              zero-filled ONCE before its first use; every call leaves it ready for the next
                              (self-resetting arrival counter). One workspace per concurrently used stream. */
    int64_t workspace_bytes;
    float *energy_f32;     /* optional device scalar: (float)(energy * energy_scale), e.g. the mean loss, written by the
                              same launch (saves the caller two elementwise kernels per evaluation); needs workspace  */
    double energy_scale;
    /* Split evaluation (no reference counterpart; the slab-parallel path, diffnet_amd/slab.py): the marched axis (y in 2-D, z in 3-D) is
     * cut into strips by the launch plan.  strip_select 1 launches only the first and the last strip -- the node layers next to the two
     * faces across the marched axis are complete after it, so their exchange with the neighbouring ranks can start --, 2 launches all the
     * other strips; 0 (default) all of them.  The two launches write disjoint parts of `out`.  accumulate_sums != 0: the final scalars
     * are added to what `energy` / `sumsq` (both required then) already hold and energy_f32 is formed from the running energy: launch 1
     * with accumulate_sums = 0, then launch 2 with 1, on one stream, gives the sums of the whole mesh in a fixed order. */
    int32_t strip_select, accumulate_sums;
    /* defer_sums != 0: the launch leaves its per-workgroup partial sums in the workspace and writes none of energy / sumsq / energy_f32;
     * dn_poisson_finish_sums(mesh, args, stream) adds them up (one small kernel, fixed order) on ANY stream ordered after the launch --
     * e.g. a side stream, under the next launch: the in-kernel final reduction is a ~3 us serial tail at the end of a ~56 us launch
     * (its last workgroup waits for every other one), the deferred one overlaps the next evaluation.  The workspace must not be handed
     * to another launch before the finish kernel has run (one workspace per evaluation in flight). */
    int32_t defer_sums;
    /* fold_prev != NULL (round 4): the arguments of an EARLIER dn_poisson_apply call on the same mesh that ran with defer_sums (its
     * partial sums still lie in ITS workspace).  This launch's first workgroup adds them up and writes that call's energy / sumsq /
     * energy_f32 -- what dn_poisson_finish_sums would do -- before it starts its own strip: the final reduction of evaluation k leaves
     * the critical path (no tail at the end of launch k, no extra kernel, no event) and rides at the start of launch k + 1, where one
     * of ~2000 workgroups doing 1-2 us of extra work delays nothing.  A loop therefore gets the loss of step k when launch k + 1 has
     * run (a training loop only logs it); the last evaluation is closed with dn_poisson_finish_sums.  The earlier call's partial count
     * and layout are derived from THIS call's mesh: it must have been made with an identical dn_mesh (batch included) on the same
     * stream.  A split launch (strip_select 2) left without strips runs the one-workgroup finish kernel for it.  Kernels without the path (anything
     * but the 2-D closed-form Q1 kernel and the 3-D Q1 two-element node-owner kernel) return DN_E_UNSUPPORTED.  Read at call time only. */
    const struct dn_poisson_args *fold_prev;
    /* f_is_load != 0 (round 4): `f` does not hold nodal forcing values but the ASSEMBLED load vector b_a = sum_e sum_g w_g N_a(g) f_g
     * (the rule's own weights, no wscale / beta: what this operator returns as -out for u = 0, alpha = 0, beta = 1, wscale = 1, no
     * conditions).  The forcing of a sample does not change from one training step to the next (the reference re-interpolates it to
     * the Gauss points every step, e.g. IBN/poisson-2d/parametric/IBN_2D.py:128-130), so it can be assembled once when the dataset is
     * placed on the device; the operator then spends one FMA per node on it instead of the element's forcing arithmetic (a fifth of
     * the 3-D Q1 kernel's time): out_a -= beta wscale b_a,  sum W f u = sum_a u_a b_a -- equal to the nodal-forcing result to rounding.
     * Only the 3-D Q1 two-element node-owner kernel (even nx, 2-point rule, constant-value uint8 / fp32 masks) takes it so far; every
     * other launch returns DN_E_UNSUPPORTED. */
    int32_t f_is_load;
} dn_poisson_args;

int dn_abi_version(void);
/* Human-readable build info ("gfx950 hipcc <ver> ..."), static storage. */
const char *dn_build_info(void);

/* Measurement probe, no reference counterpart: out = a * b + c over n floats (n % 4 == 0, 16-byte aligned arrays) as a plain streaming
 * kernel -- three arrays read once, one written once: the access mix of the fused energy loss + gradient without its halo rows, its
 * reduction and its arithmetic.  bench.py runs it over the arrays of the timed launches and reports the rate as
 * roofline.stream_ceiling.  mode: bit 0 non-temporal stores, bit 1 non-temporal loads, bits 2.. the form (0 one 16-byte vector per
 * thread, 1 blocks of four vectors per thread, 2 the same with 2048 persistent workgroups). */
int dn_probe_stream(const float *a, const float *b, const float *c, float *out, int64_t n, int32_t mode, void *stream);
/* Second probe: the MARCHING access pattern of the fused 2-D kernel without its arithmetic (arrays (B, ny, 512) fp32): a 128-thread
 * workgroup walks a strip of R node rows row by row with `rows_ahead` (1..4) rows requested ahead of the one it consumes.  flags: bit 0
 * read one halo row on either side of the strip, bit 1 also load the dword of the node shared with the right neighbour, bit 2
 * non-temporal stores, bit 3 non-temporal vector loads, bit 4 shared node taken from the neighbouring lane (one lane per wave loads it).
 * tools/march_probe.py: which (R, rows_ahead) the memory system rewards. */
int dn_probe_march(const float *a, const float *b, const float *c, float *out, int32_t B, int32_t ny, int32_t R, int32_t rows_ahead,
                   int32_t flags, void *stream);
/* Third probe: the TILE access pattern -- a workgroup requests all rows of a tile of rows_per_tile (4 | 8 | 16) node rows plus one halo row
 * on either side at once, parks them in LDS and walks them from there (threads 256 | 512; flags bit 3 non-temporal loads, bit 6
 * consecutive tiles on one XCD). */
int dn_probe_tile(const float *a, const float *b, const float *c, float *out, int32_t B, int32_t ny, int32_t rows_per_tile, int32_t threads,
                  int32_t flags, void *stream);

/* Meshes: nsd = 2, degree 1..3 (ngp 2..4, >= 3 for degree > 1); nsd = 3, degree 1 (marching kernels) and degree 2 / 3 with ngp 3 / 4 (element
 * vectors + fixed-order gather assembly: the workspace then also holds (degree + 1)^3 floats per element and is needed for every call, with
 * or without sums; no strip_select / accumulate_sums / defer_sums in that form).  dn_poisson_workspace_bytes says what a mesh needs. */
int64_t dn_poisson_workspace_bytes(const dn_mesh *mesh);
int dn_poisson_apply(const dn_mesh *mesh, const dn_poisson_args *args, void *stream);
/* Second half of a dn_poisson_apply launch with args->defer_sums set (same mesh, same args): the final scalars from the partial sums. */
int dn_poisson_finish_sums(const dn_mesh *mesh, const dn_poisson_args *args, void *stream);

/* Which kernel and which launch geometry dn_poisson_apply takes for (mesh, args) under the current switches: a host-side query, nothing is
 * launched, no device is needed and no pointer is followed (pointers count as NULL / non-NULL and by their alignment, as in the launch).  The
 * answer comes from the function the launch itself calls (poisson_choose in csrc/poisson_fused.hip), so the two cannot drift; the same function
 * tells dn_poisson_finish_sums and a folding launch (fold_prev) how many partial sums an earlier launch left and how they are laid out.
 * Returns 0, or the DN_E_* code dn_poisson_apply would return for these arguments (DN_E_BADARG also for a NULL `out`); on an error the
 * fields decided up to that point are filled, the rest 0.  No reference counterpart (the reference has no launch plan).
 *   family           DN_POISSON_*: one value per kernel template
 *   tile             threads of a workgroup -- 2-D {T, 0}, 3-D {TX, TY} (0 for DN_POISSON_3D_Q23: fixed workgroups of 64 and 256 threads)
 *   E, R, W          elements per thread along x, element layers per strip, strips chained per workgroup (2-D closed form only, else 1)
 *   ua               2-D closed form: rows of 4 k + 1 nodes taken four elements per thread with unaligned vector accesses
 *   chunks, tiles    workgroups along x and (3-D) y;  strips: strips of the whole mesh along the marched axis
 *   launched_strips  strips this launch covers (strip_select applied; 0: the launch has nothing to do)
 *   vec, allow_e4    vector accesses of the E * degree nodes a thread owns per row are legal / rows are 16-byte aligned throughout
 *   compact          conditions the call may hold without an image: 0 none, 1 DN_MASK_BOX, 2 DN_MASK_BOX and DN_MASK_BITS (no image beside them)
 *   launched         workgroups of the launch = per-workgroup partial sums it leaves (chunks x tiles x ceil(launched_strips / W) x batch)
 *   stride           workgroups the two partial-sum arrays are laid out for: the sum-of-squares partials start `stride` doubles behind the energy partials
 *   workspace_bytes  workspace a call with sums needs at this alignment (<= dn_poisson_workspace_bytes(mesh)) */
enum {
    DN_POISSON_2D_Q1_CF = 1,      /* poisson2d_q1_cf_kernel: closed-form Q1 element, nodal / absent forcing */
    DN_POISSON_2D_Q1_RULE = 2,    /* poisson2d_q1_raw_kernel: Q1 marched per Gauss rule (f_gp, or "Q1_RULE_KERNEL") */
    DN_POISSON_2D_Q23 = 3,        /* poisson2d_kernel: Q2 / Q3 */
    DN_POISSON_3D_Q1_N1 = 4,      /* poisson3d_q1n_kernel: node-owner form, one element per thread */
    DN_POISSON_3D_Q1_T16 = 5,     /* poisson3d_q1w_kernel, T16 form: tiles 16 threads wide */
    DN_POISSON_3D_Q1_GENERIC = 6, /* poisson3d_q1w_kernel, any tile */
    DN_POISSON_3D_Q1_N2 = 7,      /* poisson3d_q1n2_kernel: node-owner form, two elements per thread */
    DN_POISSON_3D_Q1_CFZ = 8,     /* poisson3d_q1_cf_kernel: two elements per thread, closed form in z */
    DN_POISSON_3D_Q23 = 9         /* poisson3d_gen_*_kernel: element vectors + gather assembly */
};
typedef struct dn_poisson_kernel {
    int32_t family;
    int32_t tile[2];
    int32_t E, R, W, ua;
    int32_t chunks, tiles, strips, launched_strips;
    int32_t vec, allow_e4, compact;
    int64_t launched, stride, workspace_bytes;
} dn_poisson_kernel;
int dn_poisson_query(const dn_mesh *mesh, const dn_poisson_args *args, dn_poisson_kernel *out);

/* Sticky error state of the launches that used `workspace` (dn_poisson_apply, dn_fsdt_apply).  The chained-strip launch plans hand rows
 * from wave to wave through flag-guarded LDS words; every poll of such a flag is bounded so that a producer wave that never arrives
 * cannot hang the GPU.  A poll that reaches its bound is never silent: the wave adds NaN to every value it writes afterwards (its rows
 * of `out`, its partial sums, hence the launch's energy / sumsq / norms) and sets bit 0 of the workspace's error word.  This call waits
 * for `stream`, reads the word, clears it, and returns 0 or DN_E_HANDOVER (synchronous: for health checks, not for the launch path).
 * The reference has no such state: its loss bodies are synchronous torch ops (IBN/poisson-2d/parametric/IBN_2D.py:116-134). */
int dn_workspace_status(void *workspace, void *stream);

/* gauss_pt_eval (DiffNet/DiffNetFEM.py:7-18) for an arbitrary table list, and its adjoint.
 *   out[b,g,e] = sum_a tables[g][a] * in[b, node(e,a)]          (conv_nd with stride `degree`)
 * in: (B,1,*N); tables: (G, nbf^nsd) device fp32; out: (B,G,*nel). nsd in {1,2,3}, nbf in 2..4.
 * n[] = nodes per axis in (x,y,z) order (unused axes 1).  The adjoint writes every element of
 * grad_in exactly once (gather form).  Replaces the 12 gauss_pt_evaluation* wrappers
 * (DiffNet/DiffNetFEM.py:143-174) and their autograd backward (conv_backward_input). */
int dn_gauss_pt_eval_fwd(const float *in, const float *tables, float *out, int32_t batch, int32_t nsd,
                         const int32_t n[3], int32_t nbf, int32_t stride, int32_t G, void *stream);
int dn_gauss_pt_eval_bwd(const float *grad_out, const float *tables, float *grad_in, int32_t batch, int32_t nsd,
                         const int32_t n[3], int32_t nbf, int32_t stride, int32_t G, void *stream);

/* Q1_2D_vector_assembly / Q1_3D_vector_assembly (e8_2d_poisson_mms.py:85-90, e8_3d_poisson_mms.py:78-87)
 * generalised to any degree: out[b, node] (+)= sum over the elements e and local ids a that map to node
 * of r_split[b,a,e], in the reference's a-ascending order.  accumulate = 0 overwrites `out`.
 * dn_assemble_bwd is its adjoint: grad_split[b,a,e] = grad_out[b, node(e,a)]. */
int dn_assemble(const float *r_split, float *out, int32_t batch, int32_t nsd, const int32_t n[3], int32_t nbf,
                int32_t stride, int32_t accumulate, void *stream);
int dn_assemble_bwd(const float *grad_out, float *grad_split, int32_t batch, int32_t nsd, const int32_t n[3],
                    int32_t nbf, int32_t stride, void *stream);

/* Winding-number inside/outside field: compute_winding_nodes of IBN/poisson-2d/parametric/IBN_2D.py:89-104.
 * points, normals: (B, Npts, 2); nodes: (2, Ny, Nx) node coordinates (xx, yy); out: (B, 1, Nx, Ny) in the reference's
 * (Nx, Ny) order: out[b,0,ix,iy] = sum_p ((p - q).n_p) / (4 pi |p - q|_1)^3 with q = nodes[:, iy, ix]. */
int dn_winding_nodes(const float *points, const float *normals, const float *nodes, float *out, int32_t batch,
                     int32_t npts, int32_t ny, int32_t nx, void *stream);

/* General winding-number field of a point cloud, 2-D or 3-D, with area weights, on a flat list of queries shared by all samples:
 *   w[b,q] = scale * sum_p area[b,p] * ((x_p - q) . n_p) / dist(x_p - q)^power
 * dim = 2 or 3; metric 0: dist is the L1 norm (the reference's compute_winding_torch, compute_winding_gpts and
 * compute_winding_nodes), metric 1: the Euclidean norm (the true generalised winding number at power = dim and
 * scale = 1/(2 pi) or 1/(4 pi)); power = 2 or 3.
 *   points, normals (B, npts, dim); area (B, npts) or NULL (= 1); queries (dim, nq), coordinate-major;
 *   out (B, nq) fp32 and / or mask (B, nq) bytes, mask = (w > threshold) compared in the kernel: at least one of the two.
 * tile = queries per thread: 0 picks it from the problem size (dn_winding_field_tile(batch, nq) returns that choice: the
 * largest of 1, 2, 4 that leaves the chip about four waves per SIMD; DN_E_BADARG for batch < 1 or nq < 1), 1, 2 or 4 force it
 * (a workgroup of 256 threads owns 256 * tile queries and stages the cloud through LDS 256 points at a time).  Each query sums
 * its points in index order in one chain, so the result is bitwise the same for every tile and grid; no atomics.  A point that
 * coincides with a query gives inf or nan, as in the reference.  Not differentiable: nothing is saved for a backward pass.
 * DN_E_BADARG before any launch: a NULL points / normals / queries, both outputs NULL, dim, metric, power or tile outside
 * the values above, batch outside 1..65535, npts < 1, nq < 1 or nq > 16777215 * 256 * tile (the grid's limit). */
int dn_winding_field_tile(int32_t batch, int64_t nq);
int dn_winding_field(const float *points, const float *normals, const float *area, const float *queries, float *out,
                     uint8_t *mask, int32_t batch, int32_t npts, int64_t nq, int32_t dim, int32_t metric, int32_t power,
                     float scale, float threshold, int32_t tile, void *stream);

/* Vector-Jacobian product of dn_winding_field with respect to the cloud (queries are constants), same layouts and parameters.  With
 * d = x_p - q, num = d . n_p, a_p = 1 without area and the cotangent g = grad_field (B, nq):
 *   L2 (metric 1): inv = r^-power, r = |d|_2,     dinv_i = -power d_i r^-(power + 2)
 *   L1 (metric 0): inv = s^-power, s = sum |d_i|, dinv_i = -power sgn(d_i) s^-(power + 1),  sgn(0) = 0 (torch's convention)
 *   grad_area[b,p]      = scale     sum_q g num inv                       (B, npts); needs `area`
 *   grad_normals[b,p,i] = scale a_p sum_q g d_i inv                       (B, npts, dim)
 *   grad_points[b,p,i]  = scale a_p sum_q g (n_i inv + num dinv_i)        (B, npts, dim)
 * Any of the three outputs may be NULL, not all.  This differentiates the reference forms the forward covers (compute_winding_torch,
 * examples/eiqonal/single_instance/02_differentiable_winding_number.py:15-30, plain differentiable torch there; compute_winding_gpts and
 * compute_winding_nodes in 2-D).
 * A workgroup owns 256 points of one sample and the queries pass through LDS 256 at a time; the query range is split over
 * `slices` workgroups (0: dn_winding_field_vjp_slices(batch, npts, nq), the count that gives each of the 256 CUs about 64 workgroups, at
 * most the number of 256-query chunks and at most 1024; a larger request than chunks is clamped to the chunks).  Order: inside a chunk
 * fp32 chains from zero in query order, chunks added in float64, slices added in float64 in index order by a second small launch, one
 * rounding to float32; no atomics.  Results are bitwise repeatable for a given slice count and the same whichever outputs are
 * requested; across slice counts the last bits may differ (the forward's bits do not depend on its tile).  With more than one
 * effective slice the launch needs `workspace` of dn_winding_field_vjp_workspace_bytes(batch, npts, dim, slices) =
 * slices * batch * npts * (1 + 2 dim) * 8 bytes, 8-byte aligned; it is not read between calls.  A point that coincides with a query
 * gives inf or nan, as in the forward.
 * All checks come before any launch.  DN_E_BADARG: a NULL points / normals / queries / grad_field, all three outputs NULL, grad_area
 * without area, dim, metric or power outside the forward's values, batch outside 1..65535, npts < 1, nq < 1, slices < 0 or > 1024
 * (dn_winding_field_vjp_slices: batch, npts or nq < 1; ..._workspace_bytes: also slices < 1).  DN_E_WORKSPACE: more than one effective
 * slice and a NULL or too small workspace. */
int dn_winding_field_vjp_slices(int32_t batch, int32_t npts, int64_t nq);
int64_t dn_winding_field_vjp_workspace_bytes(int32_t batch, int32_t npts, int32_t dim, int32_t slices);
int dn_winding_field_vjp(const float *points, const float *normals, const float *area, const float *queries,
                         const float *grad_field, float *grad_points, float *grad_normals, float *grad_area, void *workspace,
                         int64_t workspace_bytes, int32_t batch, int32_t npts, int64_t nq, int32_t dim, int32_t metric, int32_t power,
                         float scale, int32_t slices, void *stream);

/* DiffNetFDM stencil derivatives (DiffNet/DiffNetFDM.py:158-199): out = Corr( conv2d(g_padded, kernel9) ) with
 * g_padded (B,1,ny+2,nx+2) replicate-padded by the caller as in the reference, out (B,1,ny,nx), kernel9 a HOST pointer to
 * the 3x3 correlation kernel (row-major), and the reference's dense correction matmul (:63-119) reduced to what it does:
 * along `axis` (0 = x: columns, 1 = y: rows) the two boundary lines become a*d[edge] + b*d[edge+-1].
 * dn_fdm_stencil_bwd is the adjoint (gradient wrt g_padded). */
int dn_fdm_stencil_fwd(const float *g_padded, float *out, int32_t batch, int32_t ny, int32_t nx, const float *kernel9,
                       int32_t axis, float a, float b, void *stream);
int dn_fdm_stencil_bwd(const float *grad_out, float *grad_g_padded, int32_t batch, int32_t ny, int32_t nx,
                       const float *kernel9, int32_t axis, float a, float b, void *stream);

/* ---- fused FSDT (Mindlin) plate residuals ---------------------------------------------------------------------
 * Replaces the loss body of examples/elasticity/single_instance/e1_plate_bending_fsdt.py:128-232 (9 Gauss-point
 * evaluations of w, phi_x, phi_y, the constitutive combinations, three weak-form residuals, their assembly, the
 * Dirichlet rows and the three Frobenius sums) by one launch; mesh: nsd = 2, degree 1..3, ngp 2..4.
 *   fields (B,1,ny,nx) fp32; bc_mask marks Dirichlet nodes (fp32: >= 0.5 as in the script, u8: != 0; NULL = none);
 *   on those nodes the inputs are replaced by bc_field[k] (or bc_value[k] when the pointer is NULL) and so are the
 *   rows of the k-th residual.  A44, A55 include the shear correction K_s; wscale = (hx/2)(hy/2).
 *   out[k]: assembled residual k (may be NULL); sumsq: 3 doubles, sum of squares of each residual field
 *   (deterministic in-kernel reduction; needs the workspace, zero-filled once before first use).
 * The operator is the gradient of the plate energy (symmetric Jacobian): the VJP wrt the fields is the same call on
 * the masked cotangents with q = 0 and zero Dirichlet values. */
typedef struct dn_fsdt_args {
    const float *w, *phi_x, *phi_y;
    const void *bc_mask;
    int32_t mask_is_u8, mask_batched;
    const float *bc_field[3];
    int32_t bc_field_batched[3];
    float bc_value[3];
    float D11, D12, D22, D66, A44, A55, q;
    float wscale;
    float *out[3];
    double *sumsq;
    void *workspace;
    int64_t workspace_bytes;
    const float *in_scale; /* optional: 3 device floats, field k is multiplied by in_scale[k] as it is loaded (before the
                              Dirichlet substitution) -- lets the VJP of the three norms run without a scaling pass */
    float *norms;          /* optional: 3 device floats, norms[k] = sqrt(sum of squares of residual k) written by the same launch -- the
                              three Frobenius norms of e1_plate_bending_fsdt.py:230-232 without a torch op behind the kernel */
    const float *in_num;   /* optional, both or neither (not with in_scale): field k is multiplied by in_num[k] / in_den[k] as it is */
    const float *in_den;   /* loaded, by 0 where in_den[k] <= 0: the VJP of the norms is this call on the saved residuals with
                              in_num = cotangents of the norms, in_den = the norms (torch's zero subgradient at a zero norm) */
    int32_t defer_sums;    /* (round 4) non-zero: the launch leaves its per-workgroup partial sums of squares in `workspace` and does NOT form
                              sumsq / norms (the arrival protocol and the last workgroup's reduction are 4.5-6.6 us at the end of every launch:
                              a third of the 1025^2 Q2 launch at one sample); sumsq and norms are ignored.  The value is the pair's TICKET: it is
                              left in the workspace next to the partials, and any launch that reduces in the kernel clears it */
    int32_t den_ticket;    /* with den_workspace: the ticket the producer was launched with; if the workspace holds another one (some other reducing
                              dn_fsdt_apply launch used it in between) the scales, this call's outputs and the norms come out NaN.  Only FSDT
                              launches clear the ticket: other entry points must not be handed the producer's workspace in between (the Python
                              layer gives FSDT, Poisson and Stokes launches separate workspaces) */
    const void *den_workspace; /* (round 4) the `workspace` of an earlier launch with defer_sums on the same mesh, stream and launch plan: every
                              workgroup of THIS launch reduces those partials (fixed order: bitwise the sums the producer would have formed)
                              and uses their square roots where it would have read in_den (in_num required, in_den NULL); if sumsq / norms of
                              this call are non-NULL they receive the producer's sums / norms.  The loss + gradient of the plate is then two
                              launches with no reduction on the critical path of either */
} dn_fsdt_args;
int64_t dn_fsdt_workspace_bytes(const dn_mesh *mesh);
int dn_fsdt_apply(const dn_mesh *mesh, const dn_fsdt_args *args, void *stream);

/* ---- fused 2-D Stokes (PSPG) residuals -------------------------------------------------------------------------
 * Replaces the residual body of the three-field Stokes scripts of the reference:
 * examples/stokes/single_instance/e2_stokes_ldc_resmin.py:151-240, e1_stokes_mms_resmin.py:122-217,
 * e1_stokes_mms_resmin_loss2.py:158-247, and the Stokes stage of the Navier-Stokes scripts
 * (examples/navier-stokes/single_instance/e2_ns_fps_resmin.py:193 calc_residuals_stokes, e2_ns_fps_af_bcmask.py:199,
 * e2_ns_fps_af_pc.py:234, b1_stokes_ns_resmin_base.py:181): Dirichlet substitution, 9 Gauss-point evaluations, three weak
 * forms, three assemblies, the Dirichlet rows and the three Frobenius sums, in ONE launch.  Mesh: nsd = 2, degree 1, ngp 2..4.
 *   u~ = where(bc1, u_bc, u), v~ = where(bc2, v_bc, v), p~ = where(bc3, p_bc, p)      (mask: fp32 >= 0.5, u8 != 0)
 *   R1_a = sum_e sum_g J w_g [ visco (Nx_a u~_x + Ny_a u~_y) - Nx_a p~ - N_a f1 ]
 *   R2_a = sum_e sum_g J w_g [ visco (Nx_a v~_x + Ny_a v~_y) - Ny_a p~ - N_a f2 ]
 *   R3_a = sum_e sum_g J w_g [ N_a (u~_x + v~_y) + pspg (Nx_a p~_x + Ny_a p~_y) ]
 *   R_k = where(bc_k, value_k, R_k)   (Dirichlet rows take the VALUE, as in the scripts),  J = wscale
 * Fields (B,1,ny,nx) fp32.  Per field k: bc_mask[k] NULL (no condition) or an fp32 / u8 image, shared (1,1,ny,nx) or per sample;
 * the value is bc_field[k] (shared or per sample) or the constant bc_value[k].  Forcing k: f_gp[k] at the Gauss points
 * (Bf,G,nely,nelx) with Bf = 1 (f_batched 0) or B, else the constant f_value[k] (0: none).
 * out[k] may be NULL; sumsq (3 doubles) / norms (3 floats, sqrt of sumsq): fixed-order fp64 reduction in the kernel, needs
 * `workspace` (zero-filled once before first use, dn_stokes_workspace_bytes; one per stream, not shared with other operators).
 * in_num / in_den (both or neither): field k is scaled by in_num[k] / in_den[k] as it is loaded (0 where in_den[k] <= 0).
 * transpose != 0: the adjoint J_R^T = S J_R S, S = diag(1, 1, -1) -- p is negated as it is loaded and R3 before its Dirichlet
 * rows, the forcing is dropped and the Dirichlet values are zero (bc_field / bc_value / f_gp / f_value are ignored).  The VJP of
 * the three norms is this launch on the residuals with in_num = cotangents of the norms, in_den = the norms.
 * Coefficients of the scripts: e2_stokes_ldc_resmin / e1_stokes_mms_resmin_loss2: visco = 1/Re, pspg = h^2 Re / 12, J = (h/2)^2;
 * e1_stokes_mms_resmin: visco = Re; the Navier-Stokes Stokes stage: visco = 1/Re, pspg = hx hy Re / 12, J = 1, no forcing.
 * DN_E_UNSUPPORTED for nsd != 2, degree != 1, ngp outside 2..4; DN_E_BADARG for NULL fields, no output at all, in_num without
 * in_den, flags outside {0, 1} or a bc_field without its mask; nothing is launched then. */
typedef struct dn_stokes_args {
    const float *u, *v, *p;
    const void *bc_mask[3];
    int32_t mask_is_u8[3];
    int32_t mask_batched[3];
    const float *bc_field[3];
    int32_t bc_field_batched[3];
    float bc_value[3];
    const float *f_gp[2];
    int32_t f_batched[2];
    float f_value[2];
    float visco, pspg, wscale;
    int32_t transpose;
    float *out[3];
    double *sumsq;
    float *norms;
    const float *in_num, *in_den;
    void *workspace;
    int64_t workspace_bytes;
} dn_stokes_args;
int64_t dn_stokes_workspace_bytes(const dn_mesh *mesh);
int dn_stokes_apply(const dn_mesh *mesh, const dn_stokes_args *args, void *stream);

/* ---- fused 2-D Navier-Stokes (VMS) residuals and their VJP --------------------------------------------------------
 * Replaces the nonlinear residual body of the Navier-Stokes scripts of the reference:
 * examples/navier-stokes/single_instance/e1_ns_ldc_resmin.py:147-308 (calc_tau, calc_residuals), e2_ns_fps_resmin.py:293
 * calc_residuals_ns, e2_ns_fps_af_bcmask.py:299, e2_ns_fps_af_pc.py:341, b1_stokes_ns_resmin_base.py, e4_stokes_ns_cases.py:
 * Dirichlet substitution, the Gauss-point evaluations, the variational-multiscale weak forms, three assemblies, the Dirichlet rows
 * and the three Frobenius sums, in ONE launch.  Mesh: nsd = 2, degree 1 (the scripts' Laplacian terms vanish), ngp 2..4.
 *   u~ = where(bc1, u_bc, u), v~ = where(bc2, v_bc, v), p~ = where(bc3, p_bc, p)      (mask: fp32 >= 0.5, u8 != 0)
 *   at every Gauss point, from u~, v~, p~:  a1 = u u_x + v u_y,  a2 = u v_x + v v_y,  d = u_x + v_y,
 *     r1 = a1 + p_x - f1,  r2 = a2 + p_y - f2,
 *     tau_m = 1 / sqrt(Gx u^2 + Gy v^2 + cinv visco^2 (Gx^2 + Gy^2)),  tau_c = sqrt(...) / (gx^2 + gy^2),
 *     gx = 2 / tau_h[0], gy = 2 / tau_h[1], Gx = gx^2, Gy = gy^2 (float32, as the scripts' calc_tau); tau is DETACHED (no gradient)
 *   T1_a = N a1 + visco (Nx u_x + Ny u_y) - Nx p - N f1 + tau_m (u Nx + v Ny) r1 - tau_m N (r1 u_x + r2 u_y)
 *          - tau_m^2 r1 (r1 Nx + r2 Ny) + tau_c Nx d
 *   T2_a = N a2 + visco (Nx v_x + Ny v_y) - Ny p - N f2 + tau_m (u Nx + v Ny) r2 - tau_m N (r1 v_x + r2 v_y)
 *          - tau_m^2 r2 (r1 Nx + r2 Ny) + tau_c Ny d
 *   T3_a = N d + tau_m (Nx r1 + Ny r2)
 *   R_k = assemble(sum_g wscale w_g T_k),  R_k = where(bc_k, value_k, R_k)   (Dirichlet rows take the VALUE, as in the scripts)
 * Fields (B,1,ny,nx) fp32.  Masks, value fields and forcing as in dn_stokes_args.  out[k] may be NULL; sumsq (3 doubles) / norms
 * (3 floats): fixed-order fp64 reduction in the kernel, needs `workspace` (zero-filled once before first use, dn_ns_workspace_bytes;
 * one per stream, not shared with other operators).  out[k] is bitwise independent of the batch it is computed in; sumsq / norms are
 * reproducible for a given mesh and batch size, but their fp32 per-lane partial sums follow the launch plan, which depends on B, so
 * they (and, through in_den, the gradients of the norms) may differ in the last bits between batch sizes -- as in dn_stokes_apply.
 * vjp != 0: the vector-Jacobian product at the linearisation point (u, v, p) -- with the same masks, values and forcing -- of the
 * cotangents cot[0..2] of (R1, R2, R3), tau held fixed: out[k] = d/d(field k) sum_j <cot_j, R_j>, zero on field k's Dirichlet nodes
 * (the cotangent of a Dirichlet row of R_j is dropped).  in_num / in_den (both or neither, VJP only): cot[k] is scaled by
 * in_num[k] / in_den[k] as it is loaded (0 where in_den[k] <= 0); the VJP of the three norms is this launch on the saved residuals
 * with in_num = cotangents of the norms, in_den = the norms.
 * Coefficients of the scripts: visco = 1/Re, wscale = (hx/2)(hy/2), tau_h = (hx, hy) the mesh spacing, cinv = 36.
 * DN_E_UNSUPPORTED for nsd != 2, degree != 1, ngp outside 2..4; DN_E_BADARG for NULL fields, no output at all, in_num without
 * in_den, in_num outside the VJP mode, a VJP without its three cotangents, flags outside {0, 1}, tau_h not positive or a bc_field
 * without its mask; nothing is launched then. */
typedef struct dn_ns_args {
    const float *u, *v, *p;
    const void *bc_mask[3];
    int32_t mask_is_u8[3];
    int32_t mask_batched[3];
    const float *bc_field[3];
    int32_t bc_field_batched[3];
    float bc_value[3];
    const float *f_gp[2];
    int32_t f_batched[2];
    float f_value[2];
    float visco, wscale;
    float tau_h[2];
    float cinv;
    int32_t vjp;
    const float *cot[3];
    float *out[3];
    double *sumsq;
    float *norms;
    const float *in_num, *in_den;
    void *workspace;
    int64_t workspace_bytes;
} dn_ns_args;
int64_t dn_ns_workspace_bytes(const dn_mesh *mesh);
int dn_ns_apply(const dn_mesh *mesh, const dn_ns_args *args, void *stream);

/* ---- fused 2-D scalar transport (SUPG) residual and its VJP ------------------------------------------------------------
 * Replaces the residual body of the scalar transport scripts of the reference under examples/poisson/single_instance/:
 * e17_adv_diff_2d_resmin.py:99-171 (AdvDiff2d.loss), e3_st_mms_resmin.py:97-173 (SpaceTimeHeat.loss_resmin) and
 * e18_allen_cahn_ice_melt.py:77-151 (AllenCahnIceMelt.loss): the two Dirichlet substitutions, the Gauss-point evaluations, the
 * stabilised weak form, the assembly, the Dirichlet rows and the sum of squares, in ONE launch.  Mesh: nsd = 2, degree 1, ngp 2..4.
 *   u~ = where(bc2, value2, where(bc1, value1, u))      (mask: fp32 >= 0.5, u8 != 0; where both hold condition 2 wins on u)
 *   at every Gauss point, from u~ and the nodal coefficient nu (NULL: 1) evaluated there:
 *     adv = adv[0] u_x + adv[1] u_y,   r(u) = react[0] + react[1] u + react[2] u^2 + react[3] u^3,   f = f_gp or f_value
 *     A = adv + r(u) - f,   B = kappa[0] nu u_x + tau adv[0] (adv - f),   C = kappa[1] nu u_y + tau adv[1] (adv - f)
 *   R = assemble(sum_g wscale w_g (N_a A + Nx_a B + Ny_a C))
 *   R = where(bc, value, R)   (Dirichlet rows take the VALUE, as in the scripts; where both conditions hold: value1 if
 *                              r_first_wins (e3), else value2 (e17, e18))
 * u (B,1,ny,nx) fp32.  nu (1 | B,1,ny,nx).  Per condition k: bc_mask[k] NULL (no condition) or an fp32 / u8 image, shared
 * (1,1,ny,nx) or per sample; the value is bc_field[k] (shared or per sample) or the constant bc_value[k].  Forcing: f_gp at the Gauss
 * points (Bf,G,nely,nelx) with Bf = 1 (f_batched 0) or B, else the constant f_value.  out may be NULL; sumsq (1 double) / norm
 * (1 float, sqrt of sumsq): fixed-order fp64 reduction in the kernel, needs `workspace` (zero-filled once before first use,
 * dn_transport_workspace_bytes; one per stream, not shared with other operators).  out is bitwise independent of the batch it is
 * computed in and of the launch plan; sumsq / norm are reproducible for a given mesh and batch size.
 * vjp != 0: the vector-Jacobian product at the linearisation point u -- with the same masks, values and coefficients -- of the
 * cotangent cot of R: out = d/du <cot, R>, zero on the Dirichlet nodes (the cotangent of a Dirichlet row of R is dropped):
 *     q = L + tau (adv[0] L_x + adv[1] L_y),  A' = L r'(u),  B' = adv[0] q + kappa[0] nu L_x,  C' = adv[1] q + kappa[1] nu L_y
 * with (L, L_x, L_y) the cotangent evaluated like a field; the forcing is not read, and u only where react[1..3] != 0.
 * in_num (VJP only): cot is scaled by in_num[0] as it is loaded -- the VJP of the loss sum R^2 is this launch on the saved R with
 * in_num = 2 gout; with in_den also: by in_num[0] / in_den[0] (0 where in_den[0] <= 0) -- the VJP of the norm, in_den = the norm.
 * Coefficients of the scripts (h: element size), wscale = (h/2)^2:
 *   e17: adv = (cos pi/6, sin pi/6), kappa = (D, D), tau = 1 / (2 |adv| / h + 4 D / h^2), react = 0, value1 = 1, value2 = 0;
 *   e3:  adv = (0, 1), kappa = (D, 0), tau = h / 2, react = 0, value1 = the field u0, r_first_wins;
 *   e18: adv = (0, 1), kappa = (D Cn^2, D Cn^2), tau = 0, react = (-D^2 k, 2 D^2 A, -6 D^2 A, 4 D^2 A), value1 = the field u0.
 * DN_E_UNSUPPORTED for nsd != 2, degree != 1, ngp outside 2..4; DN_E_BADARG for a NULL u, no output at all, in_den without in_num,
 * in_num outside the VJP mode, a VJP without its cotangent, flags outside {0, 1} or a bc_field without its mask; DN_E_WORKSPACE
 * for a reduction without a large enough workspace; nothing is launched then. */
typedef struct dn_transport_args {
    const float *u;
    const float *nu;
    int32_t nu_batched;
    int32_t r_first_wins;
    const void *bc_mask[2];
    int32_t mask_is_u8[2];
    int32_t mask_batched[2];
    const float *bc_field[2];
    int32_t bc_field_batched[2];
    float bc_value[2];
    const float *f_gp;
    int32_t f_batched;
    float f_value;
    float adv[2];
    float kappa[2];
    float tau;
    float react[4];
    float wscale;
    int32_t vjp;
    const float *cot;
    float *out;
    double *sumsq;
    float *norm;
    const float *in_num, *in_den;
    void *workspace;
    int64_t workspace_bytes;
} dn_transport_args;
int64_t dn_transport_workspace_bytes(const dn_mesh *mesh);
int dn_transport_apply(const dn_mesh *mesh, const dn_transport_args *args, void *stream);

/* ---- fused 2-D strong-form least-squares loss and its gradient ------------------------------------------------------------
 * Replaces the loss bodies of the strong-form scripts of the reference, the only callers of its second-derivative Gauss-point
 * evaluations: examples/burgers/single_instance/01_2d_space_time.py:73-96 (Burgers.loss: space-time Burgers on Q2, y is time) and
 * examples/poisson/single_instance/10_manufactured_strong_form_higher_order.py:69-96 (Poisson.loss: strong-form Poisson on Q3) -- the
 * two Dirichlet substitutions, 4-5 Gauss-point evaluations, the weighted sum of squares and the autograd backward through all of it,
 * in ONE launch that reads u once.  Mesh: nsd = 2, degree 1..3, ngp 2..4 (>= 3 for degree > 1), (n - 1) % degree == 0.
 *   u~ = u after bc[0] then bc[1] (applied in order, as in dn_poisson_args: where both hold, condition 2's value is used)
 *   at every Gauss point, from u~:   r_g = ax u_x + ay u_y + b u u_x + dxx u_xx + dyy u_yy + fs f_g        (x is the fastest axis)
 *   sum    = sum_{b,e,g} W_g r_g^2,   W_g = gpw_g * wscale        (one double, unscaled; fixed-order fp64 reduction in the kernel)
 *   grad_a = out_scale * s * sum_{e contains a} sum_g 2 W_g r_g ( ax Nx_a + ay Ny_a + b (N_a u_x + u Nx_a) + dxx Nxx_a + dyy Nyy_a )
 *   grad is zero on the Dirichlet nodes;  s = in_scale[0] when that device float is given, else 1.
 * u, grad (B,1,ny,nx) fp32.  The forcing f_g is the nodal field f (1 | B,1,ny,nx) interpolated with the basis, or f_gp at the Gauss
 * points (Bf,G,nely,nelx) with Bf = 1 (f_batched 0) or B, or the constant f_value; f and f_gp exclude each other.  Conditions:
 * DN_MASK_F32 / DN_MASK_U8 images, shared or per sample, constant value or value field.  d2basis[ig][ib] = phi''_ib(xi_ig) in
 * reference coordinates (dn_mesh carries no second-derivative table); the kernel scales it by scale[d]^2.  For degree 1 the
 * second-derivative terms vanish identically and no work is spent on them.
 * Either grad or sum may be NULL (not both).  sum needs `workspace` (zero-filled once before first use, dn_strongform_workspace_bytes;
 * every call leaves it ready for the next; one per stream, not shared with other operators).  No atomics on the data path: grad is
 * bitwise independent of the batch it is computed in and of the launch plan ("PLAN_FSDT" "T,R" overrides the plan, as for the FSDT
 * element form); sum is reproducible for a given mesh, batch size and plan.
 * Coefficients of the scripts, both with wscale = 1 and out_scale = 1 / (B nel) (torch.mean of the gpw-weighted sums, no Jacobian):
 *   01_2d_space_time: (ax, ay, b, dxx, dyy, fs) = (0, 1, 1, 0, 0, 0) -- its loss evaluates u_xx but never uses it; the viscous form
 *   is dxx = -nu with nu = 0.01 / pi;  10_manufactured_strong_form_higher_order: (0, 0, 0, 1, 1, 1) with the nodal forcing.
 * DN_E_UNSUPPORTED for degree outside 1..3, ngp outside 2..4 (or 2 with degree > 1), DN_MASK_BITS / DN_MASK_BOX conditions (expand
 * them: dn_unpack_mask_bits); DN_E_BADARG for nsd != 2, (n - 1) % degree != 0, a NULL u, no output at all, f together with f_gp,
 * flags outside {0, 1} or a value field without its mask; DN_E_WORKSPACE for sum without a large enough workspace; nothing is
 * launched then. */
typedef struct dn_strongform_args {
    const float *u;        /* (B,1,ny,nx) nodal field                                   */
    const float *f;        /* (B | 1,1,ny,nx) nodal forcing or NULL                     */
    const float *f_gp;     /* (Bf,G,nely,nelx) forcing at Gauss points or NULL          */
    int32_t f_batched;     /* 0: one forcing for the whole batch                        */
    float f_value;         /* the forcing when f and f_gp are NULL                      */
    dn_dirichlet bc[2];    /* applied in order                                          */
    float ax, ay, b, dxx, dyy, fs;
    float wscale, out_scale;
    float d2basis[4][4];
    const float *in_scale; /* optional: one device float                                */
    float *grad;           /* (B,1,ny,nx) or NULL                                       */
    double *sum;           /* device scalar or NULL                                     */
    void *workspace;
    int64_t workspace_bytes;
} dn_strongform_args;
int64_t dn_strongform_workspace_bytes(const dn_mesh *mesh);
int dn_strongform_apply(const dn_mesh *mesh, const dn_strongform_args *args, void *stream);

/* ---- fused 2-D first-order-system least-squares loss (u, mx, my) and its three gradients ------------------------------------
 * Replaces the loss body of the three-field strong-form script of the reference,
 * examples/poisson/single_instance/11_manufactured_strong_form_two_dofs.py:37-71 (Poisson.loss on u and the flux (mx, my)) -- the two
 * Dirichlet substitutions of u, eleven Gauss-point evaluations, the weighted sums of squares and the autograd backward through all
 * of it, in ONE launch that reads every field once.  Mesh: nsd = 2, degree 1..3, ngp 2..4 (>= 3 for degree > 1), (n - 1) % degree == 0.
 *   u~ = u after bc[0] then bc[1] (applied in order, as in dn_strongform_args: where both hold, condition 2's value is used);
 *   the conditions act on u only, mx and my are free.  At every Gauss point (x is the fastest axis):
 *   qx = mx - nu u~_x,   qy = my - nu u~_y,   d = mx_x + my_y + fs f_g
 *   sum       = sum_{b,e,g} W_g ( wq (qx^2 + qy^2) + wd d^2 ),   W_g = gpw_g * wscale   (one double, unscaled; fixed-order fp64 reduction)
 *   grad_u_a  = out_scale * s * sum -2 W_g wq nu (qx Nx_a + qy Ny_a)                    (zero on the Dirichlet nodes)
 *   grad_mx_a = out_scale * s * sum  2 W_g (wq qx N_a + wd d Nx_a)
 *   grad_my_a = out_scale * s * sum  2 W_g (wq qy N_a + wd d Ny_a)                      s = in_scale[0] when that device float is given, else 1
 * u, mx, my are fp32 node images (ny,nx) per sample, sample b of each at its pointer + b * field_stride elements: field_stride is
 * ny*nx for three separate (B,1,ny,nx) tensors and 3*ny*nx for channels of one packed (B,3,ny,nx) tensor, which is then read without
 * a copy.  grad_u, grad_mx, grad_my likewise with grad_stride; any of them may be NULL.  nu is the constant nu_value or a nodal field
 * (1 | B,1,ny,nx) interpolated with the basis.  The forcing f_g is the nodal field f (1 | B,1,ny,nx) interpolated with the basis,
 * or f_gp at the Gauss points (Bf,G,nely,nelx) with Bf = 1 (f_batched 0) or B, or the constant f_value; f and f_gp exclude each
 * other.  Conditions: DN_MASK_F32 / DN_MASK_U8 images, shared or per sample, constant value or value field.
 * Any subset of the three gradients and sum may be requested (not none).  sum needs `workspace` (zero-filled once before first use,
 * dn_fosls_workspace_bytes; every call leaves it ready for the next; one per stream, not shared with other operators).  No atomics on
 * the data path: the gradients are bitwise independent of the batch they are computed in and of the launch plan ("PLAN_FSDT" "T,R"
 * overrides the plan, as for dn_strongform_apply); sum is reproducible for a given mesh, batch size and plan.
 * The script: degree 1, ngp 2, wq = wd = fs = 1, wscale = 1, out_scale = 1 / (B nel) (torch.mean of the gpw-weighted sums, no
 * Jacobian), nu and f nodal fields, conditions `> 0.5` with values 1 and 0.
 * DN_E_UNSUPPORTED for degree outside 1..3, ngp outside 2..4 (or 2 with degree > 1), DN_MASK_BITS / DN_MASK_BOX conditions (expand
 * them: dn_unpack_mask_bits); DN_E_BADARG for nsd != 2, (n - 1) % degree != 0, a NULL u, mx or my, no output at all, f together with
 * f_gp, flags outside {0, 1}, a value field without its mask, or field_stride (grad_stride, when a gradient is requested) smaller
 * than ny*nx; DN_E_WORKSPACE for sum without a large enough workspace; nothing is launched then. */
typedef struct dn_fosls_args {
    const float *u;        /* sample b at u + b * field_stride, (ny,nx)                 */
    const float *mx;
    const float *my;
    int64_t field_stride;  /* elements between samples of u, mx, my                     */
    const float *nu;       /* (B | 1,1,ny,nx) nodal coefficient or NULL                 */
    int32_t nu_batched;    /* 0: one coefficient field for the whole batch              */
    float nu_value;        /* the coefficient when nu is NULL                           */
    const float *f;        /* (B | 1,1,ny,nx) nodal forcing or NULL                     */
    const float *f_gp;     /* (Bf,G,nely,nelx) forcing at Gauss points or NULL          */
    int32_t f_batched;     /* 0: one forcing for the whole batch                        */
    float f_value;         /* the forcing when f and f_gp are NULL                      */
    dn_dirichlet bc[2];    /* applied to u in order                                     */
    float wq, wd, fs;
    float wscale, out_scale;
    const float *in_scale; /* optional: one device float                                */
    float *grad_u;         /* sample b at grad_u + b * grad_stride, or NULL             */
    float *grad_mx;
    float *grad_my;
    int64_t grad_stride;   /* elements between samples of the gradients                 */
    double *sum;           /* device scalar or NULL                                     */
    void *workspace;
    int64_t workspace_bytes;
} dn_fosls_args;
int64_t dn_fosls_workspace_bytes(const dn_mesh *mesh);
int dn_fosls_apply(const dn_mesh *mesh, const dn_fosls_args *args, void *stream);

/* ---- fused 2-D Helmholtz energy and weak-form residual -------------------------------------------------------------------
 * Replaces the loss body the two Helmholtz scripts of the reference share, examples/poisson/single_instance/14_helmholtz_mms.py:37-63
 * and 14_helmholtz_ddelta.py:37-63 (Poisson.loss: gpw (0.5 (nu |grad u|^2 - khh^2 u^2) - u f), the Poisson energy plus a reaction
 * term) -- the two Dirichlet substitutions, five Gauss-point evaluations, the weighted sum and the autograd backward through all of
 * it -- in ONE launch that reads u once.  Mesh: nsd = 2, degree 1..3, ngp 2..4 (>= 3 for degree > 1), (n - 1) % degree == 0.
 *   u~ = u after bc[0] then bc[1] (applied in order, as in dn_poisson_args: where both hold, condition 2's value is used)
 *   energy = sum_{b,e,g} W_g ( c nu_g |grad u~_g|^2  -  cr sg_g u~_g^2  -  fs u~_g f_g ),            W_g = gpw_g * wscale
 *   out_a  = out_scale * zero_on_dirichlet( sum_{e contains a} sum_g W_g ( alpha nu_g gradN_a . grad u~_g
 *                                                                          - gamma sg_g N_a u~_g  -  beta N_a f_g ) )
 *   sumsq  = sum over (b, nodes) of (out / out_scale)^2
 * u, out (B,1,ny,nx) fp32.  nu is NULL (nu == 1) or a nodal field (1 | B,1,ny,nx) interpolated with the basis; sg is the constant
 * sigma_value, or the nodal field sigma (1 | B,1,ny,nx) interpolated the same way (sigma_value is ignored then).  The forcing f_g is
 * the nodal field f (1 | B,1,ny,nx) interpolated with the basis, or f_gp at the Gauss points (Bf,G,nely,nelx) with Bf = 1 (f_batched
 * 0) or B, or the constant f_value; f and f_gp exclude each other.  Conditions: DN_MASK_F32 / DN_MASK_U8 images, shared or per sample,
 * constant value or value field.  energy, sumsq: device doubles, unscaled (fixed-order fp64 reduction in the kernel); each may be
 * NULL, but at least one of out, energy, sumsq must be given.
 * It replaces, per call:
 *   - the energy and its gradient (alpha = 2c, gamma = 2cr, beta = fs).  The scripts: c = cr = 0.5, sigma_value = khh^2, fs = 1,
 *     wscale = 1, out_scale = 1 / (B nel) (torch.mean of the gpw-weighted sums, no Jacobian), nu and f nodal fields;
 *   - the weak-form residual R with sumsq = sum R^2 (alpha = gamma = beta = 1), the well-posed loss once sigma exceeds the lowest
 *     eigenvalue and the energy is indefinite (what the *_resmin scripts do for Poisson, e8_2d_poisson_mms.py:92-150);
 *   - the backward of the residual loss: the operator is symmetric, so the gradient of sum R^2 is a second launch on u := 2R with
 *     no forcing (beta = 0, f = f_gp = NULL, f_value = 0) and the same masks with value 0 (no value field).
 * Energy or sumsq needs `workspace` (zero-filled once before first use, dn_helmholtz_workspace_bytes =
 * 4160 + 16 * chunks * nely * B bytes with nely = (ny - 1) / degree, Q = (nx - 1) / degree + 1 and chunks = 1 for Q <= 64, else
 * ceil((Q - 1) / 63); every call leaves it ready for the next; one per stream, not shared with other operators).  No atomics on the
 * data path: out is bitwise independent of the batch it is computed in and of the launch plan ("PLAN_FSDT" "T,R" overrides the plan,
 * as for dn_strongform_apply); energy and sumsq are reproducible for a given mesh, batch size and plan.
 * DN_E_UNSUPPORTED for degree outside 1..3, ngp outside 2..4 (or 2 with degree > 1), DN_MASK_BITS / DN_MASK_BOX conditions (expand
 * them: dn_unpack_mask_bits); DN_E_BADARG for nsd != 2, (n - 1) % degree != 0, a NULL u, no output at all, f together with f_gp,
 * flags outside {0, 1} or a value field without its mask; DN_E_WORKSPACE for energy or sumsq without a large enough workspace;
 * nothing is launched then. */
typedef struct dn_helmholtz_args {
    const float *u;        /* (B,1,ny,nx) nodal field                                   */
    const float *nu;       /* (B | 1,1,ny,nx) nodal coefficient or NULL (nu == 1)       */
    const float *sigma;    /* (B | 1,1,ny,nx) nodal reaction coefficient or NULL        */
    const float *f;        /* (B | 1,1,ny,nx) nodal forcing or NULL                     */
    const float *f_gp;     /* (Bf,G,nely,nelx) forcing at Gauss points or NULL          */
    int32_t nu_batched;    /* 0: one coefficient field for the whole batch              */
    int32_t sigma_batched; /* same for sigma                                            */
    int32_t f_batched;     /* same for f / f_gp                                         */
    float sigma_value;     /* the reaction coefficient when sigma is NULL               */
    float f_value;         /* the forcing when f and f_gp are NULL                      */
    dn_dirichlet bc[2];    /* applied in order                                          */
    float c, cr, fs;       /* the energy's coefficients                                 */
    float alpha, gamma, beta; /* out's coefficients                                     */
    float wscale, out_scale;
    float *out;            /* (B,1,ny,nx) or NULL                                       */
    double *energy;        /* device scalar: sum (unscaled) or NULL                     */
    double *sumsq;         /* device scalar: sum over nodes of (out/out_scale)^2 or NULL */
    void *workspace;
    int64_t workspace_bytes;
} dn_helmholtz_args;
int64_t dn_helmholtz_workspace_bytes(const dn_mesh *mesh);
int dn_helmholtz_apply(const dn_mesh *mesh, const dn_helmholtz_args *args, void *stream);

/* ---- fused 2-D stabilised eikonal weak-form residual and its VJP ----------------------------------------------------------
 * Replaces the domain term of the eikonal scripts of the reference, examples/eiqonal/parametric/10_fixed_bc.py:127-216
 * (loss_eikonal) and examples/eiqonal/single_instance/e01_curve_reconstruction.py:452-558 (loss4) -- the two Dirichlet substitutions,
 * three Gauss-point evaluations, the stabilised weak form, its assembly, the zeroed Dirichlet rows and the Frobenius norm -- in one
 * launch.  Mesh: nsd = 2, degree 1..3, ngp 2..4 (>= 3 for degree > 1), (n - 1) % degree == 0.
 *   u~ = u after bc[0] then bc[1] (applied in order, as in dn_poisson_args: where both hold, condition 2's value is used)
 *   R_a = zero_on_dirichlet( sum_{e contains a} sum_g W_g ( tau u~_g gradN_a . grad u~_g + sq N_a |grad u~_g|^2 - N_a f_g ) )
 *   W_g = gpw_g * wscale;   sumsq = sum over (b, nodes) of R^2;   norm = sqrt(sumsq)
 * The scripts: sq = 1 + tau, f = 1, wscale = (hx/2)(hy/2); tau = 0, sq = 1 is the unstabilised N (|grad u|^2 - 1).
 * vjp = 0: out = R.  The forcing f_g is the nodal field f (1 | B,1,ny,nx) interpolated with the basis, or f_gp at the Gauss points
 * (Bf,G,nely,nelx) with Bf = 1 (f_batched 0) or B, or the constant f_value; f and f_gp exclude each other.
 * vjp = 1: out = J(u~)^T cot', the pullback of cot (B,1,ny,nx) through R at u, zero on the Dirichlet nodes; cot' is cot times
 * in_num[0] (divided by in_den[0] where given; 0 where in_den[0] == 0), read as zero on the Dirichlet nodes.  The forcing is not read.
 * With cot = R, in_num -> 2 this is the gradient of sumsq; with in_num -> 1 and in_den -> the norm of the forward launch, of the norm:
 * loss plus gradient are two launches with nothing in between.  in_num, in_den: device floats.
 * u, out (B,1,ny,nx) fp32.  Conditions: DN_MASK_F32 / DN_MASK_U8 images, shared or per sample, constant value or value field.
 * sumsq: device double; norm: device float (fixed-order fp64 reduction in the kernel); each may be NULL, but at least one of out,
 * sumsq, norm must be given.  sumsq or norm needs `workspace` (zero-filled once before first use, dn_eikonal_workspace_bytes =
 * 4160 + 16 * chunks * nely * B bytes with nely = (ny - 1) / degree, Q = (nx - 1) / degree + 1 and chunks = 1 for Q <= 64, else
 * ceil((Q - 1) / 63); every call leaves it ready for the next; one per stream, not shared with other operators).  No atomics on the
 * data path: out is bitwise independent of the batch it is computed in and of the launch plan ("PLAN_FSDT" "T,R" overrides the plan,
 * as for dn_strongform_apply); sumsq and norm are reproducible for a given mesh, batch size and plan.
 * DN_E_UNSUPPORTED for degree outside 1..3, ngp outside 2..4 (or 2 with degree > 1), DN_MASK_BITS / DN_MASK_BOX conditions (expand
 * them: dn_unpack_mask_bits); DN_E_BADARG for nsd != 2, (n - 1) % degree != 0, a NULL u, no output at all, f together with f_gp,
 * vjp without cot, in_den without in_num, in_num with vjp = 0, flags outside {0, 1} or a value field without its mask;
 * DN_E_WORKSPACE for sumsq or norm without a large enough workspace; nothing is launched then. */
typedef struct dn_eikonal_args {
    const float *u;        /* (B,1,ny,nx) nodal field (vjp: the linearisation point)    */
    dn_dirichlet bc[2];    /* applied in order                                          */
    const float *f;        /* (B | 1,1,ny,nx) nodal forcing or NULL                     */
    const float *f_gp;     /* (Bf,G,nely,nelx) forcing at Gauss points or NULL          */
    int32_t f_batched;     /* 0: one forcing field for the whole batch                  */
    float f_value;         /* the forcing when f and f_gp are NULL (the scripts: 1)     */
    float tau;             /* stabilisation: tau u grad N . grad u                      */
    float sq;              /* weight of N |grad u|^2 (the scripts: 1 + tau)             */
    float wscale;
    int32_t vjp;           /* 0: residual, 1: its VJP                                   */
    const float *cot;      /* vjp: (B,1,ny,nx) cotangent of R                           */
    const float *in_num;   /* vjp: device float, cot is scaled by in_num[0]; or NULL    */
    const float *in_den;   /* vjp: device float, ... and divided by in_den[0]; or NULL  */
    float *out;            /* (B,1,ny,nx) or NULL                                       */
    double *sumsq;         /* device scalar: sum of out^2 or NULL                       */
    float *norm;           /* device scalar: its square root or NULL                    */
    void *workspace;
    int64_t workspace_bytes;
} dn_eikonal_args;
int64_t dn_eikonal_workspace_bytes(const dn_mesh *mesh);
int dn_eikonal_apply(const dn_mesh *mesh, const dn_eikonal_args *args, void *stream);

/* ---- fused 3-D stabilised eikonal weak-form residual and its VJP ----------------------------------------------------------
 * The 3-D twin of dn_eikonal_apply: the domain term of examples/eiqonal/single_instance/05_3d_sphere_loss4.py:269-425 (loss4;
 * 04_3d_sphere_recon.py::loss is its unstabilised form) -- the two Dirichlet substitutions, four Gauss-point evaluations, the
 * stabilised weak form, its assembly, the zeroed Dirichlet rows and the Frobenius norm -- in one launch.  It takes the same
 * dn_eikonal_args.  Mesh: nsd = 3, degree 1, ngp 2..4.
 *   u~ = u after bc[0] then bc[1] (where both hold, condition 2's value is used)
 *   at a Gauss point:  A = sq |grad u~|^2 - f,   (B, C, D) = tau u~ grad u~
 *   R_a = zero_on_dirichlet( sum_{e contains a} sum_g W_g ( N_a A + Nx_a B + Ny_a C + Nz_a D ) ),   W_g = gpw_g * wscale
 *   sumsq = sum over (b, nodes) of R^2;   norm = sqrt(sumsq)
 * The scripts: sq = 1 + tau, f = 1, wscale = (hx/2)(hy/2)(hz/2); 04 is tau = 0, sq = 1, f = h.
 * vjp = 0: out = R.  The forcing f_g is the nodal field f (1 | B,1,nz,ny,nx) interpolated with the basis, or f_gp at the Gauss points
 * (Bf,G,nelz,nely,nelx) with Bf = 1 (f_batched 0) or B and the Gauss points in the order of gauss_pt_evaluation on a 3-D mesh
 * (g = (kg * ngp + jg) * ngp + ig, x fastest), or the constant f_value; f and f_gp exclude each other.
 * vjp = 1: out = J(u~)^T cot', the pullback of cot (B,1,nz,ny,nx) through R at u, zero on the Dirichlet nodes: with cot' evaluated like
 * a field (L, grad L),  A' = tau grad L . grad u~,  (B', C', D') = 2 sq L grad u~ + tau u~ grad L  in the same flux form.  cot' is cot
 * times in_num[0] (divided by in_den[0] where given; 0 where in_den[0] == 0, NaN is propagated), read as zero on the Dirichlet nodes.
 * The forcing is not read.  With cot = R, in_num -> 2 this is the gradient of sumsq; with in_num -> 1 and in_den -> the norm of the
 * forward launch, of the norm: loss plus gradient are two launches with nothing in between.
 * u, out (B,1,nz,ny,nx) fp32.  Conditions: DN_MASK_F32 / DN_MASK_U8 images, shared or per sample, constant value or value field.
 * sumsq: device double; norm: device float (fixed-order fp64 reduction in the kernel); each may be NULL, but at least one of out,
 * sumsq, norm must be given.  sumsq or norm needs `workspace` (zero-filled once before first use; every call leaves it ready for the
 * next; one per stream, not shared with other operators) of dn_eikonal3d_workspace_bytes =
 *   4160 + 8 * chunks * tiles * strips * B bytes,   tiles(n, T) = 1 for n <= T, else ceil((n - 1) / (T - 1)),
 *   chunks = tiles(nx, TX), tiles = tiles(ny, TY), strips = ceil(nelz / R), nelz = nz - 1, for the launch plan (TX, TY, R):
 *   TX = 16; TY = the first of 4, 8, 12, 16 with the largest ny / (tiles(ny, TY) * TY) + 0.002 * TY; R = 32, halved while R > 4 and
 *   chunks * tiles * B * ceil(nelz / R) < 1024, then at most nelz.  "PLAN3D" "TX,TY,E,R" (2 <= TX, TY; TX * TY a multiple of 64, at
 *   most 256; R >= 1; E is ignored: one element per thread) overrides the plan and with it the size.
 * No atomics on the data path: out is bitwise independent of the batch it is computed in and of the launch plan; sumsq and norm are
 * reproducible for a given mesh, batch size and plan.  Samples of 2^30 nodes or more are DN_E_UNSUPPORTED (32-bit in-sample offsets).
 * DN_E_UNSUPPORTED for degree other than 1, ngp outside 2..4, DN_MASK_BITS / DN_MASK_BOX conditions (expand them:
 * dn_unpack_mask_bits); DN_E_BADARG for nsd != 3, a NULL u, no output at all, f together with f_gp, vjp without cot, in_den without
 * in_num, in_num with vjp = 0, flags outside {0, 1}, a value field without its mask or an unknown mask kind; DN_E_WORKSPACE for sumsq
 * or norm without a large enough workspace; nothing is launched then.  dn_eikonal_apply keeps refusing nsd = 3. */
int64_t dn_eikonal3d_workspace_bytes(const dn_mesh *mesh);
int dn_eikonal3d_apply(const dn_mesh *mesh, const dn_eikonal_args *args, void *stream);

/* ---- gradient of the Poisson losses with respect to the nodal coefficient and forcing ------------------------------------
 * Replaces what autograd does for the coefficient in the topology optimisation of the reference,
 * examples/poisson/single_instance/16_topopt.py:119-195 (loss = 0.5 nu grad u . grad v - v f with nu from the network, compliance
 * = -u f): backward through the Gauss-point evaluations of nu, u and f and the elementwise integrand, in ONE launch.
 * The gradient of the energy with respect to u is linear in (nu, f); this operator is the transpose of that map:
 *     g_nu[a] = a_nu * s * sum_{e contains a} sum_g W_g N_a(g) grad v_g . grad u~_g
 *     g_f [a] = a_f  * s * sum_{e contains a} sum_g W_g N_a(g) v_g                      W_g = gpw_g * wscale,  s = in_scale[0] or 1
 * u~ is u after bc[0], bc[1] (applied in order, as in dn_poisson_args); v (B,1,*N) is read as ZERO on every Dirichlet node; v NULL:
 * v = u~ (Dirichlet values included).  g_nu, g_f: (B,1,*N), one value per node and sample, either may be NULL (not both).
 *   energy loss  s_l sum W (c nu |grad u~|^2 - u~ f):   d/dnu = g_nu (v NULL, a_nu = s_l c),  d/df = g_f (v NULL, a_f = -s_l)
 *   residual R = Z (K_nu u~ - F f), cotangent lambda:   d<lambda,R>/dnu = g_nu (v = lambda, a_nu = 1),  d/df = g_f (v = lambda, a_f = -1)
 *   compliance-style functionals: g_f alone.
 * in_scale: optional device float multiplied into both outputs (the upstream grad_output without a host synchronisation).
 * Mesh: degree 1, ngp 2..4; nsd = 2 (the marching kernel of dn_transport_apply) or nsd = 3 (a plain one-thread-per-node form:
 * correct and deterministic, not optimised).  Conditions: DN_MASK_F32 / DN_MASK_U8 images (both of the same format when there are
 * two), shared or per sample, constant value or value field.  No workspace, no reduction, no atomics: every node is written once with
 * the same additions in the same order under any launch plan and batch size -- the outputs are bitwise reproducible and bitwise
 * independent of the batch they are computed in.
 * DN_E_UNSUPPORTED for degree > 1, ngp outside 2..4, DN_MASK_BITS / DN_MASK_BOX conditions (expand them: dn_unpack_mask_bits) or two
 * images of different formats; Gauss-point forcing has no nodal gradient and is not an argument.  DN_E_BADARG for a NULL u, no output
 * at all, flags outside {0, 1} or a value field without its mask; nothing is launched then. */
typedef struct dn_coef_grad_args {
    const float *u;        /* (B,1,*N) nodal field                                      */
    const float *v;        /* (B,1,*N) second field or NULL (v = u~)                    */
    dn_dirichlet bc[2];    /* applied in order                                          */
    float a_nu, a_f, wscale;
    const float *in_scale; /* optional: one device float                                */
    float *g_nu;           /* (B,1,*N) or NULL                                          */
    float *g_f;            /* (B,1,*N) or NULL                                          */
} dn_coef_grad_args;
int dn_poisson_coef_grad(const dn_mesh *mesh, const dn_coef_grad_args *args, void *stream);

/* ---- batched matrix-free conjugate gradients for the Q1 Poisson problem: the vector side ------------------------------------
 * The reference has no linear solve of its own: it trains on the loss, and where it wants the discrete solution it reaches for outside
 * linear algebra (examples/poisson/single_instance/e8_2d_poisson_mms.py:60-67,143-146 loads an ILU factor from a .mat file).  Together
 * with dn_poisson_apply (q = Z K_nu p: alpha = 1, f absent, homogeneous conditions) these entries are a Jacobi-preconditioned CG solve (with
 * dn_poisson_pcg and dn_poisson_mg further down: a multigrid-preconditioned one) of
 * Z (K_nu u~ - F f) = 0 for a whole batch without a host round trip per iteration; composed from torch ops an iteration is about a dozen
 * launches and a synchronisation for its scalars.
 *
 * dn_poisson_diag: the inverse diagonal of K_nu, one launch, no workspace, every node written once with a fixed order of additions
 * (bitwise reproducible and independent of the batch size):
 *     diag_a = wscale * sum_{e contains a} sum_g gpw_g nu_g |grad N_a(g)|^2        nu_g = sum_b N_b(g) nu_b, as in dn_poisson_apply
 *     dinv_a = 0           on a node of either condition's mask and wherever diag_a == 0 (a node surrounded by nu = 0: no equation)
 *     dinv_a = 1 / diag_a  elsewhere (unit != 0: 1 elsewhere -- the unpreconditioned solve)
 * nu: (B,1,*N), (1,1,*N) with nu_batched = 0, or NULL (nu = 1).  bc: only mask, mask_kind and mask_batched are read (DN_MASK_F32 /
 * DN_MASK_U8 images, shared or per sample, the two may differ in format).  Mesh: nsd 2 or 3, degree 1, ngp 2..4.
 * DN_E_UNSUPPORTED for degree > 1, ngp outside 2..4, nsd outside {2, 3}, samples of 2^30 nodes or more and DN_MASK_BITS / DN_MASK_BOX
 * conditions (expand them: dn_unpack_mask_bits); DN_E_BADARG for a NULL mesh, args or dinv, fewer than 2 nodes on an axis, B outside
 * 1..65535, an unknown mask kind or flags outside {0, 1}; nothing is launched then. */
typedef struct dn_poisson_diag_args {
    const float *nu;       /* (B,1,*N), (1,1,*N) or NULL (nu == 1)                      */
    int32_t nu_batched;
    dn_dirichlet bc[2];
    float wscale;
    int32_t unit;          /* 1: dinv = 1 on the free nodes                             */
    float *dinv;           /* (B,1,*N)                                                  */
} dn_poisson_diag_args;
int dn_poisson_diag(const dn_mesh *mesh, const dn_poisson_diag_args *args, void *stream);

/* dn_poisson_cg: the vector phases of one PCG iteration over flat arrays of `batch` samples of n floats (sample b starts at element
 * b * n; array bases 16-byte aligned, a sample's base need not be).  Per-sample scalars live in one dn_cg_state per sample on the device.
 *     DN_CG_INIT       (q = the operator's output Z (K x0~ - F f))   r = -q,  p = dinv r,  rz = sum r (dinv r),  rr0 = rr = sum r r,
 *                      active = rr0 > atol^2,  iterations = 0,  flags = 0,  alpha = beta = 0          -- every sample
 *     DN_CG_DOT        pq = sum p q;  alpha = rz / pq if active and pq > 0, else alpha = 0; an active sample with !(pq > 0) (an operator
 *                      that is not positive definite, or a NaN) gets flags |= DN_CG_BREAKDOWN and active = 0
 *     DN_CG_UPDATE     x += alpha p,  r -= alpha q,  rz' = sum r (dinv r),  rr = sum r r;  then beta = rz' / rz,  rz = rz',
 *                      iterations += 1,  active = rr > max(tol^2 rr0, atol^2)  (a NaN rr: DN_CG_BREAKDOWN)   -- active samples only
 *     DN_CG_DIRECTION  p = dinv r + beta p                                                             -- active samples only
 * One iteration = the operator launch on p, then DOT, UPDATE, DIRECTION: 13 floats moved per node beside the operator's.
 * No array of an inactive sample is read or written by any phase but INIT (its x, r, p stay bitwise as they are even when p or q hold
 * NaN) and its scalars but alpha are left alone.  The sums are float64 sums of products of the float32 values, taken per workgroup in
 * an order that depends on the in-sample index alone and added in a fixed order by the sample's last workgroup: a sample's scalars are
 * reproducible run to run and do not depend on the batch it is solved in, on its place in it or on which samples are active.
 * workspace: dn_poisson_cg_workspace_bytes(n, batch) bytes, 64-byte aligned, zero-filled ONCE before its first use; every launch leaves
 * it ready for the next.  One workspace per concurrently used stream.  DIRECTION needs none.
 * DN_E_BADARG for NULL args, an unknown phase, n < 1, batch outside 1..65535, a NULL or misaligned array the phase uses (x: UPDATE; r,
 * dinv: all but DOT; q: all but DIRECTION; p, state: all), negative or NaN tol / atol, and a missing or too small workspace;
 * DN_E_UNSUPPORTED for n >= 2^30.  Nothing is launched then. */
enum { DN_CG_INIT = 0, DN_CG_DOT = 1, DN_CG_UPDATE = 2, DN_CG_DIRECTION = 3 };
enum { DN_CG_BREAKDOWN = 1 };
typedef struct dn_cg_state {
    double rz, rr, rr0, pq;
    float alpha, beta;
    int32_t active, iterations, flags;
    int32_t reserved[3];
} dn_cg_state;
typedef struct dn_poisson_cg_args {
    int32_t phase;         /* DN_CG_*                                                   */
    int32_t batch;
    int64_t n;             /* nodes of one sample                                       */
    float *x;              /* (B, n) the iterate                                        */
    float *r;              /* (B, n) the residual of the recurrence                     */
    float *p;              /* (B, n) the search direction                               */
    const float *q;        /* (B, n) the operator's output: Z K p (INIT: Z (K x0~ - F f)) */
    const float *dinv;     /* (B, n) or (1, n) with dinv_batched = 0                    */
    int32_t dinv_batched;
    float tol, atol;
    dn_cg_state *state;    /* (B)                                                       */
    void *workspace;
    int64_t workspace_bytes;
} dn_poisson_cg_args;
int64_t dn_poisson_cg_workspace_bytes(int64_t n, int32_t batch);
int dn_poisson_cg(const dn_poisson_cg_args *args, void *stream);

/* dn_poisson_pcg: the vector phases of a PCG iteration whose preconditioner is a PROCEDURE -- z = M r comes from memory (a multigrid
 * V-cycle, dn_poisson_mg below) where dn_poisson_cg forms dinv r inline.  Same arrays, same dn_cg_state block, same workspace
 * (dn_poisson_cg_workspace_bytes) and the same reduction and reproducibility rules as dn_poisson_cg.
 *     DN_PCG_RESID0     (q = the operator's output Z (K x0~ - F f))   r = -q,  rr0 = rr = sum r r,  rz = 0,  active = rr0 > atol^2,
 *                       iterations = 0,  flags = 0,  alpha = beta = 0                                  -- every sample
 *     DN_PCG_UPDATE     x += alpha p,  r -= alpha q,  rr = sum r r,  iterations += 1,  active = rr > max(tol^2 rr0, atol^2)
 *                       (a NaN rr: DN_CG_BREAKDOWN)                                                    -- active samples only
 *     DN_PCG_RZ         rz' = sum r z,  beta = rz' / rz (0 where rz is not positive: the first call after RESID0),  rz = rz'
 *     DN_PCG_DIRECTION  p = z + beta p  (p = z where beta == 0, whatever p held)                        -- active samples only
 * A solve: RESID0, then [z = M r, RZ, DIRECTION] and per iteration the operator launch on p, DN_CG_DOT of dn_poisson_cg (unchanged),
 * UPDATE, [z = M r, RZ, DIRECTION].  Beside the operator and the preconditioner 13 floats move per node and iteration.
 * No array of an inactive sample is read or written by any phase but RESID0 and its scalars are left alone; it adds zeros to the sums.
 * DN_E_BADARG for NULL args, an unknown phase, n < 1, batch outside 1..65535, a NULL or misaligned array the phase uses (r, q: RESID0,
 * UPDATE; x, p: UPDATE; r, z: RZ; p, z: DIRECTION; state: all), negative or NaN tol / atol, and a missing or too small workspace
 * (DIRECTION needs none); DN_E_UNSUPPORTED for n >= 2^30.  Nothing is launched then. */
enum { DN_PCG_RESID0 = 0, DN_PCG_UPDATE = 1, DN_PCG_RZ = 2, DN_PCG_DIRECTION = 3 };
typedef struct dn_poisson_pcg_args {
    int32_t phase;         /* DN_PCG_*                                                  */
    int32_t batch;
    int64_t n;             /* nodes of one sample                                       */
    float *x;              /* (B, n) the iterate                                        */
    float *r;              /* (B, n) the residual of the recurrence                     */
    float *p;              /* (B, n) the search direction                               */
    const float *q;        /* (B, n) the operator's output: Z K p (RESID0: Z (K x0~ - F f)) */
    const float *z;        /* (B, n) the preconditioned residual M r                    */
    float tol, atol;
    dn_cg_state *state;    /* (B)                                                       */
    void *workspace;
    int64_t workspace_bytes;
} dn_poisson_pcg_args;
int dn_poisson_pcg(const dn_poisson_pcg_args *args, void *stream);

/* dn_poisson_mg: the grid transfers and the smoother update of a geometric multigrid V-cycle on nested Q1 meshes, over flat batched
 * float32 nodal arrays (sample b of a level starts at element b * n_level; array bases 16-byte aligned, a sample's base need not be).
 * The operator of a level is dn_poisson_apply on that level's mesh, its inverse diagonal dn_poisson_diag.  The fine mesh has
 * fine[0..2] = (nx, ny, nz) nodes (nz = 1 in 2-D), the coarse mesh coarse[d] = (fine[d] - 1) / 2 + 1 with every fine[d] odd.  P is the
 * multilinear interpolation coarse -> fine (per axis: a fine node 2 i takes coarse node i, a fine node 2 i + 1 half of i and of i + 1),
 * Z zeroes the nodes of a level's Dirichlet image (uint8, (B,*N) or (1,*N) with mask_batched = 0, NULL: none).
 *     DN_MG_RESTRICT  c = Z_c P^T (b - q)    c: coarse (written), b, q: fine, mask: the COARSE level's image.  The fine residual is
 *                     formed on the fly; per axis the weights are 1/2, 1, 1/2, a neighbour beyond a mesh face is absent (no renormalising)
 *     DN_MG_PROLONG   x += Z_f P c           x: fine (updated), c: coarse (read), mask: the FINE level's image
 *     DN_MG_SMOOTH    x += omega dinv (b - q)      x, b, q, dinv: arrays of fine[] nodes; coarse[], c and mask are not read
 *     DN_MG_SMOOTH0   x  = omega dinv b            the first sweep from a zero guess
 * Every output node is written by exactly one thread with additions in an order that depends on the node alone, no atomics: the
 * results are bitwise reproducible and bitwise independent of the batch size and of a sample's place in the batch.
 * DN_E_BADARG for NULL args, an unknown op, nsd outside {2, 3}, batch outside 1..65535, fewer than 2 nodes on an axis (3 on a fine axis
 * of a transfer), a coarse shape that does not match the fine one, a NULL or misaligned array the op uses, flags outside {0, 1} and a
 * NaN omega; DN_E_UNSUPPORTED for samples of 2^30 nodes or more.  Nothing is launched then. */
enum { DN_MG_RESTRICT = 0, DN_MG_PROLONG = 1, DN_MG_SMOOTH = 2, DN_MG_SMOOTH0 = 3 };
typedef struct dn_poisson_mg_args {
    int32_t op;            /* DN_MG_*                                                   */
    int32_t nsd;           /* 2 or 3                                                    */
    int32_t batch;
    int32_t fine[3];       /* nx, ny, nz of the fine (SMOOTH*: the only) level          */
    int32_t coarse[3];     /* nx, ny, nz of the coarse level (transfers)                */
    float *x;              /* (B, n_f)  PROLONG, SMOOTH: updated; SMOOTH0: written      */
    const float *b;        /* (B, n_f)  RESTRICT, SMOOTH, SMOOTH0: the right-hand side  */
    const float *q;        /* (B, n_f)  RESTRICT, SMOOTH: the operator's output Z K x   */
    const float *dinv;     /* (B, n_f) or (1, n_f) with dinv_batched = 0: SMOOTH*       */
    int32_t dinv_batched;
    float *c;              /* (B, n_c)  RESTRICT: written; PROLONG: read                */
    const uint8_t *mask;   /* RESTRICT: (B|1, n_c); PROLONG: (B|1, n_f); or NULL        */
    int32_t mask_batched;
    float omega;
} dn_poisson_mg_args;
int dn_poisson_mg(const dn_poisson_mg_args *args, void *stream);

/* dn_poisson_mg_transfer: DN_MG_RESTRICT and DN_MG_PROLONG of dn_poisson_mg between meshes that need not be nested -- an axis of e
 * elements is coarsened to ceil(e / 2) elements over the same length: coarse[d] = ceil((fine[d] - 1) / 2) + 1, which is fine[d] / 2 + 1 in
 * integers, every fine[d] >= 4. Arrays, masks and the two operations' meaning as in dn_poisson_mg; P is the multilinear interpolation between the
 * two meshes, the tensor product of per-axis matrices that the CALLER supplies as device tables (16-byte aligned), both views of the
 * same float32 numbers so that RESTRICT is the transpose of PROLONG exactly:
 *     parents[d]   fine[d] entries: fine node i of axis d takes w0 of coarse node j and w1 of coarse node j + 1 (0 <= j <= coarse[d] - 2)
 *     children[d]  coarse[d] entries: coarse node j receives w[t] of fine node first + t for t < count (count <= 4; w[t] = 0 beyond)
 * With n_f = fine[d] and n_c = coarse[d], fine node i lies at the coarse coordinate i (n_c - 1) / (n_f - 1): j = floor of it,
 * rem = i (n_c - 1) - j (n_f - 1), w0 = (n_f - 1 - rem) / (n_f - 1), w1 = rem / (n_f - 1), each rounded once to float32 on the host
 * (the last fine node: j = n_c - 2, w0 = 0, w1 = 1).  On an axis with an even element count these are the weights of dn_poisson_mg;
 * one launch may mix such axes with others.  The kernels clamp every index they read from a table into the mesh, so a wrong table
 * gives wrong numbers, not a wrong address -- but the tables must have fine[d] and coarse[d] entries.
 * Same guarantees: one thread per written node, additions in an order that depends on the node alone (z, then y, then x), no atomics,
 * no workspace; bitwise reproducible and independent of the batch size.
 * DN_E_BADARG for NULL args, an op other than the two transfers, nsd outside {2, 3}, batch outside 1..65535, a fine axis of fewer than
 * 4 nodes, a coarse extent other than fine[d] / 2 + 1, a NULL or misaligned table or array the op uses, mask_batched outside {0, 1}
 * and samples of 2^30 nodes or more.  Nothing is launched then. */
typedef struct dn_mg_parent {
    int32_t j;             /* the first parent; the second is j + 1                     */
    float w0, w1;
    int32_t pad;
} dn_mg_parent;
typedef struct dn_mg_children {
    int32_t first, count;  /* fine nodes first .. first + count - 1                     */
    int32_t pad[2];
    float w[4];
} dn_mg_children;
typedef struct dn_poisson_mg_transfer_args {
    int32_t op;            /* DN_MG_RESTRICT or DN_MG_PROLONG                           */
    int32_t nsd;           /* 2 or 3                                                    */
    int32_t batch;
    int32_t fine[3];       /* nx, ny, nz of the fine level                              */
    int32_t coarse[3];     /* nx, ny, nz of the coarse level                            */
    float *x;              /* (B, n_f)  PROLONG: updated                                */
    const float *b;        /* (B, n_f)  RESTRICT: the right-hand side                   */
    const float *q;        /* (B, n_f)  RESTRICT: the operator's output Z K x           */
    float *c;              /* (B, n_c)  RESTRICT: written; PROLONG: read                */
    const uint8_t *mask;   /* RESTRICT: (B|1, n_c); PROLONG: (B|1, n_f); or NULL        */
    int32_t mask_batched;
    const dn_mg_parent *parents[3];      /* per axis x, y, z: fine[d] entries           */
    const dn_mg_children *children[3];   /* per axis x, y, z: coarse[d] entries         */
} dn_poisson_mg_transfer_args;
int dn_poisson_mg_transfer(const dn_poisson_mg_transfer_args *args, void *stream);

/* ---- fused 2-D finite-difference Poisson residual, its sums of squares and its gradient ------------------------------------
 * Replaces the loss bodies of the three DiffNetFDM scripts of the reference under examples/poisson/single_instance/:
 * 12_fdm_mms.py:76-118, 12_klsum_fdm.py:69-111 and 12_klsum_fdm_nbc.py:69-158 -- the two Dirichlet substitutions, six valid 3x3
 * conv2d calls (sobelx / sobely / sobelxx / sobelyy on u, sobelx / sobely on nu), six elementwise passes, the sum of squares or the
 * L2 norm, the two Neumann row terms of the _nbc script and the autograd backward through all of it, in ONE launch that reads u, nu
 * and f once.  No dn_mesh: a finite-difference grid has no element geometry, only B samples of ny x nx nodes (x is the fastest axis).
 *   u~ = u after bc[0] then bc[1] (applied in order, as in dn_strongform_args: where both hold, condition 2's value is used); nu and
 *   f are taken as they are.  (k * v)_i = sum over the 3x3 neighbourhood of k[dy+1][dx+1] v[y+dy][x+dx]: the VALID CORRELATION, what
 *   nn.functional.conv2d(v, k) gives; kx, ky, kxx, kyy are passed by value, row-major, and may hold any values (the class's 'fdm'
 *   weights are only what the Python layer passes by default).  On the interior, (ny-2) x (nx-2) nodes:
 *   r      = fs f + (kx * u~)(kx * nu) + (ky * u~)(ky * nu) + nu (kxx * u~ + kyy * u~)
 *   res    (B,1,ny-2,nx-2) = r
 *   sums   (B,3) float64, per sample (unscaled; fixed-order fp64 reduction in the kernel):
 *          sum r^2 | sum_x (u~[0,x] - u~[1,x])^2 | sum_x (u~[ny-1,x] - u~[ny-2,x])^2        (nbc_down / nbc_up of 12_klsum_fdm_nbc.py:137-147)
 *   grad   (B,1,ny,nx) = out_scale ( s_b d(sum r^2)/du + nbc_scale d(sums[b][1] + sums[b][2])/du ),  exactly zero on the Dirichlet nodes;
 *          s_b = in_scale[b] when that device array of B floats is given, else 1;
 *          d(sum r^2)/du_j = 2 sum_i r_i ( kx[j-i] (kx * nu)_i + ky[j-i] (ky * nu)_i + nu_i (kxx + kyy)[j-i] ) over the interior nodes i
 *          within one step of j (the hand-derived pullback: three 3x3 adjoint stencils on three per-node products).
 * nu: (B | 1,1,ny,nx) or NULL = the constant nu_value; f likewise with f_value.  Conditions: DN_MASK_F32 / DN_MASK_U8 images, shared
 * or per sample, constant value or value field.  Each of res, sums, grad may be NULL (not all).  sums needs `workspace` (zero-filled
 * once before first use, dn_fdm_poisson_workspace_bytes = 4160 + 24 ceil(nx / 60) ny B bytes; every call leaves it ready for the
 * next; one per stream, not shared with other operators).  The mean-of-squares losses of 12_klsum_fdm.py and 12_klsum_fdm_nbc.py take
 * one launch (out_scale = 1 / (B (ny-2)(nx-2)); nbc_scale = 0.1 (ny-2)(nx-2) / nx); the per-sample L2 norm of 12_fdm_mms.py two: sums
 * first, then grad with in_scale[b] = 1 / (2 sqrt(sums[b][0])) and out_scale = 1 / B.
 * A row march for wave64: 60 owner columns and two ghost lanes on either side per wave, x neighbours by cross-lane moves, strips of
 * node rows with the seams recomputed.  No atomics on the data path: res and grad are bitwise independent of the batch a sample sits
 * in and of the launch plan ("PLAN_FSDT" "T,R" overrides the plan, as for dn_strongform_apply: T = 64 x waves per workgroup, R node
 * rows per strip); sums are reproducible for a given shape and plan.  Samples of 2^30 nodes or more are DN_E_UNSUPPORTED.
 * Out of scope: the replicate-padded and corrected form of DiffNetFDM.derivative_* (dn_fdm_stencil_fwd / dn_fdm_fused_fwd serve it),
 * gradients with respect to nu and f, the L1 norm the scripts keep commented out, 3-D grids.
 * DN_E_UNSUPPORTED for DN_MASK_BITS / DN_MASK_BOX conditions (expand them: dn_unpack_mask_bits); DN_E_BADARG for ny < 3 or nx < 3,
 * B outside 1..65535, a NULL u, no output at all, a value field without its mask, an unknown mask kind or flags outside {0, 1};
 * DN_E_WORKSPACE for sums without a large enough workspace; nothing is launched then. */
typedef struct dn_fdm_poisson_args {
    int32_t B, ny, nx;     /* samples, node rows, nodes per row                         */
    const float *u;        /* (B,1,ny,nx) nodal field                                   */
    const float *nu;       /* (B | 1,1,ny,nx) coefficient or NULL (nu_value)            */
    const float *f;        /* (B | 1,1,ny,nx) forcing or NULL (f_value)                 */
    int32_t nu_batched;    /* 0: one field for the whole batch                          */
    int32_t f_batched;
    float nu_value, f_value;
    float fs;              /* the forcing coefficient                                   */
    dn_dirichlet bc[2];    /* applied in order                                          */
    float kx[9], ky[9], kxx[9], kyy[9];
    float out_scale, nbc_scale;
    const float *in_scale; /* optional: B device floats                                 */
    float *res;            /* (B,1,ny-2,nx-2) or NULL                                   */
    double *sums;          /* (B,3) device doubles or NULL                              */
    float *grad;           /* (B,1,ny,nx) or NULL                                       */
    void *workspace;
    int64_t workspace_bytes;
} dn_fdm_poisson_args;
int64_t dn_fdm_poisson_workspace_bytes(int32_t B, int32_t ny, int32_t nx);
int dn_fdm_poisson_apply(const dn_fdm_poisson_args *args, void *stream);

/* ---- fused point-cloud terms on a Q1 mesh (2-D, 3-D): u and its gradient at points, the penalty loss, its gradient ----------
 * Replaces the point terms the point-cloud scripts of the reference add to their losses -- the four "+1" neighbour gathers, the
 * bf_1d_th / bf_1d_der_th products, the weighted sums, the squares and their sums, and the autograd backward that ends in an
 * index_put with accumulation: examples/poisson/single_instance/pc_poisson_disk.py and pc_complex_immersed_background.py (loss:
 * sum (u_p - 1)^2), examples/eiqonal/parametric/10_fixed_bc.py:186-208 and single_instance/05_3d_sphere_loss4.py:345-389 (value and
 * "dot" terms), single_instance/e01_curve_reconstruction.py:270 ("match").  Of those bodies only the two Poisson scripts' are a
 * usable definition; the terms are defined by the formulas here.
 *   The points arrive classified and sorted (diffnet_amd/points.py: PointPlan): B samples of npts points each, sorted by (sample,
 *   element); T = B npts.  elem[q]: the point's element within its sample, (ez nely + ey) nelx + ex;  xi: (nsd, T), the local
 *   coordinates in [-1, 1], one array per axis (x, y[, z]);  offsets: (B nel + 1) CSR of the sorted list over (sample, element).
 *   With N0 = (1 - xi)/2, N1 = (1 + xi)/2 per axis and N_a their products over the 2^nsd nodes a of the element:
 *   u_p = sum_a N_a u_a            g_d = dscale[d] sum_a d_d N_a u_a      (dscale 1: the scripts' reference-coordinate derivative;
 *                                                                          2 / h_d: the physical gradient)
 *   values (T) = u_p,  pgrads (nsd, T) = g_d                               where asked
 *   penalty != 0:  sums[0] = w_val sum_p (u_p - t_p)^2                     t_p = target[q], or target_value when target is NULL
 *                  sums[1] = w_nrm sum_p (g . n - 1)^2                     kind DN_POINTS_DOT     (normals: (nsd, T))
 *                          = w_nrm sum_p sum_d (g_d - n_d)^2               kind DN_POINTS_MATCH;   0 for DN_POINTS_NONE
 *                  sums[2] = sums[0] + sums[1]                             (3 device doubles; fixed-order fp64 reduction in the kernel)
 *                  cot (1 + nsd, T) = c0 = 2 w_val (u_p - t_p);  c_d = 2 w_nrm (g . n - 1) n_d  |  2 w_nrm (g_d - n_d)  |  0
 *   grad != NULL:  grad (B,1,*N) = gs sum_p ( c0 N_a + sum_d c_d dscale[d] d_d N_a )  over the points of the node's adjacent elements,
 *                  gs = gscale (x gscale_dev[0] when that device float is given); with accumulate the sum is added to grad instead,
 *                  and a node whose adjacent elements hold no point is not written.  cot is then an INPUT unless the same call
 *                  computes the penalty (forward launch, then adjoint launch): any per-point cotangents of (u_p, g_d) are pulled back.
 * Forward: one thread per point.  Adjoint: one thread per node, gather form: the node's at most 2^nsd elements in the order z, y, x,
 * each element's points in stored order, one fp32 fma chain; no atomics, bitwise reproducible.  Element ids and offsets are clamped
 * into their ranges before they address anything.  npts = 0 is valid: zero sums; grad zero-filled, or left as it is under accumulate.
 * sums needs `workspace` (zero-filled once before first use, dn_points_workspace_bytes = 4160 + 16 * 1024 bytes whatever the
 * sizes; every call leaves it ready for the next; one per stream, not shared with other operators).
 * DN_E_UNSUPPORTED for a Q2 / Q3 mesh (the Python layer composes torch ops there) and for samples of 2^30 nodes or more;
 * DN_E_BADARG for a NULL mesh or args, nsd outside {2, 3}, fewer than 2 nodes on an axis, B outside 1..65535, npts < 0 or B npts
 * >= 2^31, an unknown kind, flags outside {0, 1}, nothing to compute, accumulate without grad, sums without penalty, a penalty with
 * neither sums nor cot, and, where there are points, a NULL u / elem / xi, missing normals for the kind, or an adjoint without
 * offsets or cot;  DN_E_WORKSPACE for sums without a large enough workspace.  Nothing is launched then. */
#define DN_POINTS_NONE 0
#define DN_POINTS_DOT 1
#define DN_POINTS_MATCH 2
typedef struct dn_points_args {
    const float *u;          /* (B,1,*N) nodal field (forward)                              */
    const int32_t *elem;     /* (T) sorted element ids within the sample (forward)          */
    const float *xi;         /* (nsd, T) local coordinates                                  */
    const int32_t *offsets;  /* (B nel + 1) CSR of the sorted list (adjoint)                */
    int64_t npts;            /* points per sample                                           */
    float dscale[3];         /* derivative scale per axis (x, y, z)                         */
    int32_t kind;            /* DN_POINTS_*: the normals term                               */
    int32_t penalty;         /* 1: form the penalty terms (sums and / or cot)               */
    const float *target;     /* (T) or NULL (target_value)                                  */
    float target_value;
    const float *normals;    /* (nsd, T) or NULL (DN_POINTS_NONE)                           */
    float w_val, w_nrm;
    float *values;           /* (T) or NULL                                                 */
    float *pgrads;           /* (nsd, T) or NULL                                            */
    float *cot;              /* (1 + nsd, T): written by the penalty, read by the adjoint   */
    double *sums;            /* 3 device doubles or NULL                                    */
    const float *gscale_dev; /* optional: one device float                                  */
    float gscale;
    float *grad;             /* (B,1,*N) or NULL                                            */
    int32_t accumulate;      /* 1: grad += instead of grad =                                */
    void *workspace;
    int64_t workspace_bytes;
} dn_points_args;
int64_t dn_points_workspace_bytes(const dn_mesh *mesh);
int dn_points_apply(const dn_mesh *mesh, const dn_points_args *args, void *stream);

/* ---- fused output block of the 2-D U-Net generator ----------------------------------------------------------
 * Upsample(x2, nearest) -> ZeroPad2d((1,0,1,0)) -> Conv2d(C -> 1, 4x4, padding 1, bias) -> Sigmoid
 * (DiffNet/networks/unets.py:68-74, `self.final`) without materialising the upsampled tensor.
 *   in (B,C,h,w), weight (1,C,4,4), bias (1) device pointer or NULL, out / grad_out (B,1,2h,2w); act: 1 = sigmoid, 0 = none.
 * bwd: grad_in (B,C,h,w), grad_weight (1,C,4,4), grad_bias (1); any of the three may be NULL (grad_bias needs
 * grad_weight).  `out` is the forward result (needed when act = 1).  workspace: dn_upconv_out_workspace_bytes, no
 * initialisation required.  Weight-gradient partial sums are combined in a fixed order (bitwise repeatable). */
int64_t dn_upconv_out_workspace_bytes(int64_t B, int64_t C, int64_t h, int64_t w);
int dn_upconv_out_fwd(const float *in, const float *weight, const float *bias, float *out, int64_t B, int64_t C, int64_t h,
                      int64_t w, int act, void *workspace, int64_t workspace_bytes, void *stream);
int dn_upconv_out_bwd(const float *in, const float *weight, const float *out, const float *grad_out, float *grad_in,
                      float *grad_weight, float *grad_bias, int64_t B, int64_t C, int64_t h, int64_t w, int act, void *workspace,
                      int64_t workspace_bytes, void *stream);

/* 3-D counterpart: Upsample(x2, nearest) -> Conv3d(C -> 1, 3x3x3, padding 1, bias) -> Sigmoid
 * (DiffNet/networks/wgan3d.py:88-92, `GoodGenerator.final`).  in (B,C,d,h,w), weight (1,C,3,3,3), out (B,1,2d,2h,2w);
 * arguments as for dn_upconv_out_*. */
int64_t dn_upconv3d_out_workspace_bytes(int64_t B, int64_t C, int64_t d, int64_t h, int64_t w);
int dn_upconv3d_out_fwd(const float *in, const float *weight, const float *bias, float *out, int64_t B, int64_t C, int64_t d,
                        int64_t h, int64_t w, int act, void *workspace, int64_t workspace_bytes, void *stream);
int dn_upconv3d_out_bwd(const float *in, const float *weight, const float *out, const float *grad_out, float *grad_in,
                        float *grad_weight, float *grad_bias, int64_t B, int64_t C, int64_t d, int64_t h, int64_t w, int act,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* Weight gradient of the 4x4x4 / stride 2 / padding 1 3-D convolutions and transposed convolutions of the generator
 * (DiffNet/networks/wgan3d.py:23-55):
 *     grad_weight[m][cn][kz][ky][kx] = sum_{b,i,j,k} coarse[b][m][i][j][k] * fine[b][cn][2i+kz-1][2j+ky-1][2k+kx-1]
 *   Conv3d:          coarse = grad_out (B,cout,d,h,w), fine = input    (B,cin,2d,2h,2w),  grad_weight (cout,cin,4,4,4)
 *   ConvTranspose3d: coarse = input    (B,cin,d,h,w),  fine = grad_out (B,cout,2d,2h,2w), grad_weight (cin,cout,4,4,4)
 * M (channels of `coarse`) <= 128.  Fixed-order partial sums (bitwise repeatable); workspace needs no initialisation. */
int64_t dn_conv3d_k4s2_wrw_workspace_bytes(int64_t B, int64_t CN, int64_t M, int64_t d, int64_t h, int64_t w);
int dn_conv3d_k4s2_wrw(const float *fine, const float *coarse, float *grad_weight, int64_t B, int64_t CN, int64_t M, int64_t d,
                       int64_t h, int64_t w, void *workspace, int64_t workspace_bytes, void *stream);

/* Fused InstanceNorm (affine = False, biased variance) + LeakyReLU/ReLU of the generator blocks
 * (DiffNet/networks/unets.py:13-45, autoencoders.py:7-70, wgan3d.py:23-55): x, y (n_inst, spatial) contiguous with
 * n_inst = B*C; mean, rstd (n_inst) are written by fwd and consumed by bwd.  slope: 0 = ReLU, 0.2 = LeakyReLU(0.2),
 * 1 = no activation.  With few, large instances the work of one instance is sliced over several workgroups and the
 * fp64 partial sums go through `workspace` (dn_instnorm_workspace_bytes(n_inst, spatial) bytes, 0 when not needed;
 * no initialisation required).  Results are bitwise repeatable.  bwd: grad_y may be a channel slice of a wider
 * (B, C_total, spatial) tensor, e.g. the U-Net's skip concatenation: `channels` = C of this layer and
 * grad_y_batch_stride = elements between samples (0 = contiguous). */
int64_t dn_instnorm_workspace_bytes(int64_t n_inst, int64_t spatial);
int dn_instnorm_act_fwd(const float *x, float *y, float *mean, float *rstd, int64_t n_inst, int64_t spatial, float eps,
                        float slope, void *workspace, int64_t workspace_bytes, void *stream);
int dn_instnorm_act_bwd(const float *x, const float *mean, const float *rstd, const float *grad_y, float *grad_x,
                        int64_t n_inst, int64_t spatial, float slope, int64_t channels, int64_t grad_y_batch_stride,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* 4 x 4 / stride 2 / padding 1 convolution family of the 2-D networks (no bias), NCHW fp32, on the fp32 matrix cores.
 * Replaces the arithmetic of `nn.Conv2d(cin, cout, 4, 2, 1, bias=False)` (UNetDown, DiffNet/networks/unets.py:13-24;
 * autoencoders.py:29-34) and `nn.ConvTranspose2d(cin, cout, 4, 2, 1, bias=False)` (UNetUp, unets.py:27-45; autoencoders.py:39-45)
 * in all their passes.  `fine` lives on the 2H x 2W grid, `coarse` on the H x W grid, and w[m][c][ky][kx] (m = coarse channel,
 * c = fine channel) is Conv2d's (cout, cin, 4, 4) weight and ConvTranspose2d's (cin, cout, 4, 4) weight as they stand:
 *   down: coarse[b,m,i,j] = sum w[m,c,ky,kx] fine[b,c,2i+ky-1,2j+kx-1]      Conv2d forward / ConvTranspose2d input gradient
 *   up  : fine[b,c,y,x]   = sum w[m,c,ky,kx] coarse[b,m,(y+1-ky)/2,(x+1-kx)/2]  ConvTranspose2d forward / Conv2d input gradient
 *   wrw : gw[m,c,ky,kx]   = sum coarse[b,m,i,j] fine[b,c,2i+ky-1,2j+kx-1]   weight gradient of both (deterministic two-stage sum)
 * Shapes: fine (B,C,2H,2W), coarse (B,M,H,W), w / grad_weight (M,C,4,4). */
int dn_conv2d_k4s2_down(const float *fine, const float *w, float *coarse, int64_t B, int64_t C, int64_t M, int64_t H, int64_t W,
                        void *stream);
int dn_conv2d_k4s2_up(const float *coarse, const float *w, float *fine, int64_t B, int64_t C, int64_t M, int64_t H, int64_t W,
                      void *stream);
int64_t dn_conv2d_k4s2_wrw_workspace_bytes(int64_t B, int64_t C, int64_t M, int64_t H, int64_t W);
int dn_conv2d_k4s2_wrw(const float *fine, const float *coarse, float *grad_weight, int64_t B, int64_t C, int64_t M, int64_t H,
                       int64_t W, void *workspace, int64_t workspace_bytes, void *stream);

/* 4 x 4 x 4 / stride 2 / padding 1 convolution family of the 3-D generator (no bias), NCDHW fp32, fp32 matrix cores: the `down`
 * and `up` contractions of `nn.Conv3d(cin, cout, 4, 2, 1, bias=False)` / `nn.ConvTranspose3d(cin, cout, 4, 2, 1, bias=False)`
 * (DiffNet/networks/wgan3d.py:23-55), same conventions as dn_conv2d_k4s2_*: fine (B,C,2D,2H,2W), coarse (B,M,D,H,W), w (M,C,4,4,4).
 * The weight gradient of both layers is dn_conv3d_k4s2_wrw. */
int dn_conv3d_k4s2_down(const float *fine, const float *w, float *coarse, int64_t B, int64_t C, int64_t M, int64_t D, int64_t H,
                        int64_t W, void *stream);
int dn_conv3d_k4s2_up(const float *coarse, const float *w, float *fine, int64_t B, int64_t C, int64_t M, int64_t D, int64_t H,
                      int64_t W, void *stream);
/* The same contractions with a workspace (round 4): the deep, narrow layers of the generator (128 -> 128 channels on 4^3 positions ...) fill
 * only a few position tiles, so the contraction itself is split over workgroups -- slices of fine channels (`down`) / coarse channel
 * pairs (`up`) write partial results into the workspace and a second launch adds them in slice order (deterministic).  The library
 * decides the split from the shapes; dn_conv3d_k4s2_workspace_bytes (up = 0 / 1) returns what that split needs (0: no split).  A NULL
 * workspace runs the unsplit launch, which is what dn_conv3d_k4s2_down / _up are. */
int64_t dn_conv3d_k4s2_workspace_bytes(int32_t up, int64_t B, int64_t C, int64_t M, int64_t D, int64_t H, int64_t W);
int dn_conv3d_k4s2_down_ws(const float *fine, const float *w, float *coarse, int64_t B, int64_t C, int64_t M, int64_t D, int64_t H,
                           int64_t W, void *workspace, int64_t workspace_bytes, void *stream);
int dn_conv3d_k4s2_up_ws(const float *coarse, const float *w, float *fine, int64_t B, int64_t C, int64_t M, int64_t D, int64_t H,
                         int64_t W, void *workspace, int64_t workspace_bytes, void *stream);

/* Which kernel a launch of the two families above takes: a host-side query, nothing is launched and no device is needed.  The choice is
 * computed by the function the launch itself calls ("choose", then "launch", in csrc/conv2d_k4s2.hip, conv2d_k4s2_v2.hip, conv3d_k4s2.hip
 * and conv3d_wrw.hip), so the two cannot drift; the switches "CONV2D_V1" and "CONV_WRW_WGS" act on the query as they act on the launch.
 * The answer is for 16-byte aligned tensors (a 2-D launch with a misaligned tensor takes the generation-1 kernel of the same plan).
 *   op = DN_CONV_DOWN | DN_CONV_UP | DN_CONV_WRW; B, C, M and the COARSE sizes as in the launches (3-D wrw: C = CN fine channels).
 *   gen        2-D: 1 = the im2col kernels conv2d_k4s2_{down,up,wrw}_kernel, 2 = the raw-row-tile kernels conv2d_{down,up,wrw}_v2_kernel; 3-D: 1
 *   targ       the template arguments, unused ones 0 --  2-D gen 2: down <TM, TW, NT>, up <TC, TW, NT>, wrw <TW, NT, NCW>;
 *              2-D gen 1: down <TM>, up <TC>, wrw none;  3-D: down <TM>, up <TC>, wrw <MR>
 *   nz         slices the contraction is split into (1: the kernel writes the result itself, no workspace): gridDim.z of the 2-D wrw and
 *              3-D down kernels, gridDim.z / 2 of 3-D up, gridDim.x of 3-D wrw
 *   per_slice  2-D and 3-D wrw: tiles of 64 flattened positions (b, i, j[, k]) per slice -- slice z covers positions 64 per_slice z ...
 *              (a generation-2 2-D kernel walks 64 / NT x per_slice blocks of TR x TW = NT positions instead: blocks in x fastest, then y, then sample);
 *              3-D down: fine channels per slice; 3-D up: pairs of coarse channels per slice
 *   sum_kernel the launch that adds the slices: 0 none, 1 one thread per output (conv2d_k4s2_wsum_kernel, conv3d_wsum_few_kernel,
 *              conv3d_ksum_kernel), 2 one wave per output (conv2d_k4s2_wsum_wave_kernel, conv3d_wsum_kernel)
 * dn_conv3d_k4s2_query: with_workspace != 0 describes dn_conv3d_k4s2_down_ws / _up_ws with a workspace, 0 the unsplit launch (ignored for wrw).
 * Returns 0, or the DN_E_* code the launch would return for these sizes; DN_E_BADARG for a NULL `out` or an unknown op. */
#define DN_CONV_DOWN 0
#define DN_CONV_UP 1
#define DN_CONV_WRW 2
typedef struct dn_conv_k4s2_kernel {
    int32_t gen;
    int32_t targ[3];
    int32_t nz;
    int32_t per_slice;
    int32_t sum_kernel;
} dn_conv_k4s2_kernel;
int dn_conv2d_k4s2_query(int32_t op, int64_t B, int64_t C, int64_t M, int64_t H, int64_t W, dn_conv_k4s2_kernel *out);
int dn_conv3d_k4s2_query(int32_t op, int64_t B, int64_t C, int64_t M, int64_t D, int64_t H, int64_t W, int32_t with_workspace,
                         dn_conv_k4s2_kernel *out);

/* Stride-1 "valid" k x k convolutions (k <= 7) with optional bias: the auto-encoder's stem / head layers behind an explicit
 * ReflectionPad2d (DiffNet/networks/autoencoders.py:13 `nn.Conv2d(in_channels, dim*2, 7)`, :75 `nn.Conv2d(.., out_channels, 3)`,
 * `nn.Conv2d(out_channels, out_channels, 7)`).  x (B,Ci,H,W), w (Co,Ci,K,K), y / gy (B,Co,H-K+1,W-K+1); gbias may be NULL. */
int dn_conv2d_valid_fwd(const float *x, const float *w, const float *bias, float *y, int64_t B, int64_t Ci, int64_t Co, int64_t H, int64_t W,
                        int64_t K, void *stream);
int dn_conv2d_valid_bwd_data(const float *gy, const float *w, float *gx, int64_t B, int64_t Ci, int64_t Co, int64_t H, int64_t W, int64_t K,
                             void *stream);
int dn_conv2d_valid_bwd_weight(const float *x, const float *gy, float *gw, float *gbias, int64_t B, int64_t Ci, int64_t Co, int64_t H, int64_t W,
                               int64_t K, void *stream);

/* dn_fdm_stencil_* with the replicate padding folded in (`self.pad(u)` of DiffNet/DiffNetFDM.py:128-199 becomes clamped indexing):
 * u and out are both (B,1,ny,nx); the backward pass returns the gradient on the unpadded grid (adjoint of pad + stencil + fix-up). */
int dn_fdm_fused_fwd(const float *u, float *out, int32_t batch, int32_t ny, int32_t nx, const float *kernel9, int32_t axis, float a,
                     float b, void *stream);
int dn_fdm_fused_bwd(const float *grad_out, float *grad_u, int32_t batch, int32_t ny, int32_t nx, const float *kernel9, int32_t axis,
                     float a, float b, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFNET_HIP_H */
