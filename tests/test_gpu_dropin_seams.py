"""The single-launch ("drop-in") operators -- gauss_pt_eval forward / adjoint, assemble and its adjoint, the FDM stencils, the winding
number -- against float64 at every launch seam: tile, chunk and strip boundaries, the XCD-aware block decode (nwg < 8, nwg % 8 != 0,
nwg % 8 == 0), both 3-D small-tile adjoints, the 1-D adjoint, strides other than nbf - 1 (forward and the general gather adjoint), the
grid-stride loops behind the 4096 x 256 thread cap, non-square FDM grids and winding point counts around the 256-point LDS chunk.

The comparison is a derived bound, not a chosen tolerance.  Every operator here except the winding number is a sum of products of
float32 values, so with the reference and the magnitude field A (the same operator applied to |table|, |input|, |cotangent|) both
computed in float64 from the same float32 values,
    |got - ref| <= n * 2^-24 * A        entry by entry,
where n is the number of roundings on the longest path to one output (the gamma_n bound: it holds for any summation order).  Where A is
0 (nodes that no window covers, trailing nodes) the output must be exactly 0.  Tables are random, not the mesh's: N_gp is symmetric under
exchange of the axes and under reflection, so a transposed or mirrored local index passes for it.  The CPU tests at the end show that
the bound has teeth (a float32 evaluation passes; two swapped table columns or a cotangent shifted by one element column miss it by
orders of magnitude) and pin the FDM restatement to the reference's golden vectors before it serves non-square grids.

Largest |got - ref| / (n 2^-24 A) per operator family on the MI355X (every test prints its own; run with -s):
    gauss_pt_eval 1-D                              forward 0.60    adjoint 0.53
    gauss_pt_eval 2-D, tiled and gather adjoint    forward 0.54    adjoint 0.12
    gauss_pt_eval 3-D Q1, marching and tiled       forward 0.42    adjoint 0.044
    gauss_pt_eval 3-D Q2, small tiles              forward 0.13    adjoint 0.018
    gauss_pt_eval 3-D Q3, gather and small tiles   forward 0.065   adjoint 0.0074
    gauss_pt_eval, strides other than nbf - 1      forward 0.48    adjoint 0.24
    grid-stride cases                              forward 0.56    adjoint 0.19    assemble 0.40, onto a base 0.57
    assemble                                       0.35, onto a base 0.37; its adjoint is bitwise the float64 gather
    FDM                                            values 0.30     VJPs 0.29       fused against padded: values 0 (bitwise), VJPs 0.072
    winding number                                 0.19
(the largest forward ratios come from the two-term sums of the smallest elements, where one rounding is already a third of the bound)
"""
import functools
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import dev, load, seeded

U = 2.0 ** -24            # unit roundoff of float32


# ---------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------
def bound_ratio(got, ref, A, n):
    """max |got - ref| / (n U A); an entry that differs where A == 0 gives inf (such an output has no term: it must be exactly 0)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    err, bound = (got - ref).abs(), n * U * A
    q = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    q = torch.where(torch.isfinite(got), q, torch.full_like(q, math.inf))
    return float(q.max())


RATIOS = {}


def check(family, case, **parts):
    """parts: name -> (got, ref, A, n).  Prints every ratio, then asserts each is within the bound."""
    rs = {k: bound_ratio(*v) for k, v in parts.items()}
    RATIOS[family] = max(RATIOS.get(family, 0.0), *rs.values())
    print(f"dropin-ratio {family} {case}: " + " ".join(f"{k}={r:.3g}" for k, r in rs.items()) + f" (family max so far {RATIOS[family]:.3g})")
    for k, r in rs.items():
        assert r <= 1.0, f"{family} {case} {k}: |got - ref| is {r:.3g} x the bound n 2^-24 A"
    return rs


def rnd(shape, *key):
    """seeded uniform values in (-1/2, 1/2); the seed is a function of the case alone"""
    return seeded(shape, zlib.crc32(repr(key).encode()) & 0x7FFFFFFF, -0.5)


@pytest.fixture
def switch():
    from diffnet_amd import _lib
    held = []

    def set_(key, value="1"):
        held.append(key)
        _lib.config_set(key, value)

    yield set_
    for key in held:
        _lib.config_set(key, "")


# ---------------------------------------------------------------------------------------------
# gauss_pt_eval: reference, magnitude field, counts
# ---------------------------------------------------------------------------------------------
def gpe64(x, tab, nsd, nbf, stride):
    """the conv formulation of the oracle on (G, nbf^nsd) tables: local node a = (kb nbf + jb) nbf + ib, x fastest"""
    from oracle.fem_oracle import gauss_pt_eval
    return gauss_pt_eval(x, tab.reshape((-1, 1, 1) + (nbf,) * nsd), nsd, stride)


def gpe_pair(x, tab, cot, nsd, nbf, stride):
    """forward and adjoint (autograd of the conv formulation) in the dtype of the arguments"""
    xr = x.clone().requires_grad_(True)
    y = gpe64(xr, tab, nsd, nbf, stride)
    (g,) = torch.autograd.grad(y, xr, cot)
    return y.detach(), g


def n_fwd(nsd, nbf):
    return nbf ** nsd + 1         # one element value: nbf^nsd products in one fma chain, one rounding each; + 1 slack for the terms of second order


def n_adj(nsd, nbf, G):
    # one node: at most nbf^nsd windows (stride 1; 2^nsd at the standard stride) of G products each.  Whatever the order -- one chain
    # (general gather), a chain of G per element and <= 2^nsd - 1 adds of the partial sums (tiled, standard gather), carries handed from
    # plane to plane (3-D Q1 march) -- no product passes more roundings than there are terms; + 1 as above.  No node collects more terms
    # at any stride.
    return nbf ** nsd * G + 1


@functools.lru_cache(maxsize=4)
def gpe_problem(nsd, nbf, stride, nodes, B, G):
    """nodes = (x[, y[, z]]).  float32 inputs and, computed once and left unchanged, the float64 reference and magnitude fields."""
    shape = (B, 1) + tuple(nodes[::-1])
    key = (nsd, nbf, stride, nodes, B, G)
    x, tab = rnd(shape, "x", *key), rnd((G, nbf ** nsd), "tab", *key)
    cot = rnd((B, G) + tuple((n - nbf) // stride + 1 for n in shape[2:]), "cot", *key)
    y, g = gpe_pair(x.double(), tab.double(), cot.double(), nsd, nbf, stride)
    Ay, Ag = gpe_pair(x.abs().double(), tab.abs().double(), cot.abs().double(), nsd, nbf, stride)
    return x, tab, cot, y, g, Ay, Ag


def run_gpe(family, nsd, nbf, stride, nodes, B, G, tag=""):
    from diffnet_amd import gauss_pt_eval
    x, tab, cot, y, g, Ay, Ag = gpe_problem(nsd, nbf, stride, tuple(nodes), B, G)
    xd = x.to(dev()).requires_grad_(True)
    yd = gauss_pt_eval(xd, tab.to(dev()), nsd=nsd, stride=stride)
    (gd,) = torch.autograd.grad(yd, xd, cot.to(dev()))
    case = f"nsd={nsd} nbf={nbf} stride={stride} nodes={'x'.join(map(str, nodes))} B={B} G={G}{tag}"
    if stride != nbf - 1:                        # nodes without a window exist at these strides: the exact-zero clause is exercised
        gaps = stride > nbf or any((n - nbf) % stride for n in nodes)
        assert not gaps or bool((Ag == 0).any()), case
    return check(family, case, fwd=(yd, y, Ay, n_fwd(nsd, nbf)), adj=(gd, g, Ag, n_adj(nsd, nbf, G)))


# ---------------------------------------------------------------------------------------------
# 1. 2-D tiled adjoint gpe_bwd_tiled_kernel<2, NB>: 32 x 32-element tiles stepping by 31, XCD-aware decode
# ---------------------------------------------------------------------------------------------
TILED_2D = [   # nel_x, nel_y, B, G                 tiles (x * y * B = workgroups)
    (1, 1, 1, 1),       # 1: the smallest mesh
    (33, 5, 1, 5),      # 2 x 1: nwg < 8; G not a multiple of 4
    (64, 33, 1, 9),     # 3 x 2 = 6
    (95, 32, 2, 4),     # 4 x 1 x 2 = 8: nwg % 8 == 0
    (63, 64, 3, 16),    # 2 x 3 x 3 = 18: base 2, remainder 2; the second x-tile exactly full
    (32, 63, 1, 9),     # 1 x 2
]


@pytest.mark.gpu
@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("nel_x,nel_y,B,G", TILED_2D, ids=[f"{a}x{b}_B{c}_G{d}" for a, b, c, d in TILED_2D])
def test_gpe_2d_tiled_adjoint_seams(nel_x, nel_y, B, G, deg):
    run_gpe("gpe2d", 2, deg + 1, deg, (deg * nel_x + 1, deg * nel_y + 1), B, G)


@pytest.mark.gpu
@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("nel_x,nel_y,B,G", [TILED_2D[2], TILED_2D[4]], ids=["64x33_B1_G9", "63x64_B3_G16"])
def test_gpe_2d_gather_adjoint(nel_x, nel_y, B, G, deg, switch):
    switch("GPE_GATHER")                          # gpe_bwd_std_kernel<2, NB>
    run_gpe("gpe2d", 2, deg + 1, deg, (deg * nel_x + 1, deg * nel_y + 1), B, G, " GPE_GATHER")


# ---------------------------------------------------------------------------------------------
# 2. 1-D: forward and the adjoint gpe_bwd_std_kernel<1, NB>
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("deg", [1, 2, 3])
def test_gpe_1d_forward_and_adjoint(deg):
    for nel in (1, 7, 300):
        for B in (1, 3):
            for G in (1, 3):
                run_gpe("gpe1d", 1, deg + 1, deg, (deg * nel + 1,), B, G)


# ---------------------------------------------------------------------------------------------
# 3. 3-D Q1: the marching adjoint (both instantiations) and, under GPE_TILED, the 32 x 8 x 8 tiles
# ---------------------------------------------------------------------------------------------
Q1_3D = [(16, 17, 9), (17, 16, 10), (32, 31, 18)]      # nodes x, y, z: 1 / 2 / 3 chunks, 2 / 1 / 2 tiles, 1 / 2 / 3 strips at R = 8


@pytest.mark.gpu
@pytest.mark.parametrize("tiled", [False, True], ids=["march", "GPE_TILED"])
@pytest.mark.parametrize("G", [8, 5])
@pytest.mark.parametrize("nodes", Q1_3D, ids=["x".join(map(str, s)) for s in Q1_3D])
def test_gpe_3d_q1_adjoint_seams(nodes, G, tiled, switch):
    if tiled:
        switch("GPE_TILED")
    run_gpe("gpe3d_q1", 3, 2, 1, nodes, 2, G, " GPE_TILED" if tiled else "")


# ---------------------------------------------------------------------------------------------
# 4. / 5. 3-D Q2 and Q3: small tiles (8 x 8 x 8 / 8 x 8 x 4 elements stepping by 7 / 7 / 3) and the scalar gather
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("G", [27, 5])
@pytest.mark.parametrize("nel,B", [((8, 8, 8), 1), ((9, 15, 16), 2)], ids=["8x8x8_B1", "9x15x16_B2"])
def test_gpe_3d_q2_small_tile_adjoint(nel, B, G):
    run_gpe("gpe3d_q2", 3, 3, 2, tuple(2 * n + 1 for n in nel), B, G)


Q3_3D = [   # nel, B                 tiles x * y * z * B
    ((3, 2, 4), 1),         # 1: below 512 workgroups -> gpe_bwd_std_scalar_kernel<3, 4>
    ((9, 16, 5), 2),        # 2 * 3 * 2 * 2 = 24: scalar gather
    ((9, 16, 5), 43),       # 2 * 3 * 2 * 43 = 516 (remainder 4): gpe_bwd_tiled_kernel<3, 4, true>
    ((8, 9, 8), 86),        # 1 * 2 * 3 * 86 = 516: small tiles, three in z
]


@pytest.mark.gpu
@pytest.mark.parametrize("nel,B", Q3_3D, ids=[f"{'x'.join(map(str, n))}_B{b}" for n, b in Q3_3D])
def test_gpe_3d_q3_gather_and_small_tile_adjoint(nel, B):
    run_gpe("gpe3d_q3", 3, 4, 3, tuple(3 * n + 1 for n in nel), B, 8)


# ---------------------------------------------------------------------------------------------
# 6. strides other than nbf - 1: the forward with such a stride and gpe_bwd_kernel, the general gather
# ---------------------------------------------------------------------------------------------
STRIDES = [   # nsd, nbf, stride, nodes, B, G
    (1, 2, 3, (50,), 3, 3),
    (2, 3, 1, (37, 40), 2, 5),
    (2, 4, 1, (18, 21), 1, 16),          # four windows per node and axis
    (2, 2, 3, (37, 40), 2, 4),
    (2, 4, 2, (30, 23), 2, 9),
    (3, 3, 1, (7, 8, 9), 2, 5),
    (3, 2, 2, (8, 9, 10), 1, 8),
    (3, 4, 2, (8, 10, 12), 1, 27),
]


@pytest.mark.gpu
@pytest.mark.parametrize("nsd,nbf,stride,nodes,B,G", STRIDES, ids=[f"nsd{c[0]}_nbf{c[1]}_s{c[2]}" for c in STRIDES])
def test_gpe_general_strides(nsd, nbf, stride, nodes, B, G):
    run_gpe("gpe_stride", nsd, nbf, stride, nodes, B, G)


# ---------------------------------------------------------------------------------------------
# 8. assemble (assemble_std_kernel) and its adjoint (a copy)
# ---------------------------------------------------------------------------------------------
def n_asm(nsd):
    return 2 ** nsd + 1           # a node of the standard layout lies in <= 2^nsd elements: that many adds onto the base (or onto 0); + 1 slack


@functools.lru_cache(maxsize=2)
def asm_problem(nsd, deg, nel, B):
    from oracle.fem_oracle import Oracle
    o = Oracle(nsd=nsd, fem_basis_deg=deg, domain_size=4 * deg + 1)         # only its degree and dimension enter Oracle.assemble
    nbf = deg + 1
    key = (nsd, deg, nel, B)
    rs = rnd((B, nbf ** nsd) + tuple(nel[::-1]), "rs", *key)
    node_sp = tuple(deg * n + 1 for n in nel[::-1])
    base, cot = rnd((B, 1) + node_sp, "base", *key), rnd((B, 1) + node_sp, "cot", *key)
    rr = rs.double().requires_grad_(True)
    ref = o.assemble(rr)                                      # float64 adjoint of the one-hot-table conv
    (gather,) = torch.autograd.grad(ref, rr, cot.double())
    A = o.assemble(rs.abs().double())
    return rs, base, cot, ref.detach(), A, gather.float()


def run_assemble(family, nsd, deg, nel, B):
    from diffnet_amd import ops
    rs, base, cot, ref, A, gather = asm_problem(nsd, deg, tuple(nel), B)
    r = rs.to(dev()).requires_grad_(True)
    got0 = ops.assemble(r, nsd, deg + 1)
    got1 = ops.assemble(rs.to(dev()), nsd, deg + 1, out=base.to(dev()))
    case = f"nsd={nsd} deg={deg} nel={'x'.join(map(str, nel))} B={B}"
    check(family, case, plain=(got0, ref, A, n_asm(nsd)), onto=(got1, ref + base.double(), A + base.abs().double(), n_asm(nsd)))
    (g,) = torch.autograd.grad(got0, r, cot.to(dev()))
    assert torch.equal(g.cpu(), gather), case + ": the adjoint is a copy"


ASM = [(2, (33, 5)), (2, (7, 64)), (3, (5, 3, 4)), (3, (9, 2, 7))]


@pytest.mark.gpu
@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("nsd,nel", ASM, ids=["x".join(map(str, n)) for _, n in ASM])
def test_assemble_nonsquare(nsd, nel, deg):
    run_assemble("assemble", nsd, deg, nel, 2)


# ---------------------------------------------------------------------------------------------
# 7. the grid-stride loops behind grid_for: more than 4096 x 256 = 1 048 576 threads' worth of elements / nodes
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_grid_stride_2d_q1_forward_and_adjoints(switch):
    """769 x 769 nodes, B = 2: 1 179 648 elements, 1 182 722 nodes; the sample index changes inside a thread's stride.  Forward
    (gpe_fwd_kernel<2, 2>) and the tiled adjoint, then the per-node gather adjoint gpe_bwd_std_kernel<2, 2> under GPE_GATHER."""
    run_gpe("grid_stride", 2, 2, 1, (769, 769), 2, 4)
    switch("GPE_GATHER")
    run_gpe("grid_stride", 2, 2, 1, (769, 769), 2, 4, " GPE_GATHER")


@pytest.mark.gpu
def test_grid_stride_assemble_and_adjoint():
    """the same mesh: assemble_std_kernel<2, 2> with and without out=, assemble_bwd_kernel<2, 2>"""
    run_assemble("grid_stride", 2, 1, (768, 768), 2)


@pytest.mark.gpu
def test_grid_stride_general_stride_adjoint():
    """nbf 2, stride 3, 1100 x 1000 nodes: gpe_bwd_kernel<2, 2> walks 1 100 000 nodes with 1 048 576 threads"""
    run_gpe("grid_stride", 2, 2, 3, (1100, 1000), 1, 3)


# ---------------------------------------------------------------------------------------------
# 9. FDM: replicate pad, conv2d, correction matrix -- restated in float64, matrices built here
# ---------------------------------------------------------------------------------------------
FDM_OPS = {"x": (0, 4.0, -1.0), "y": (1, 4.0, -1.0), "xx": (0, 0.0, 1.0), "yy": (1, 0.0, 1.0)}       # axis, a, b
# roundings on the longest path, read off csrc/fdm.hip (host float32 evaluations of the same formulation have no longer ones):
N_FDM_FWD = 9 + 2 + 1           # fdm_conv: 9 products in one fma chain; a * d + b * dn: a product and an add (or one fma); + 1 slack.  (The two
#                                 stencils of a boundary value are 2 * 9 terms, but no term passes both chains: 9 + 2, not 2 * 9 + 3.)
N_FDM_PAD_ADJ = 9 + 3 + 1       # fdm_bwd_kernel: 9 taps in one fma chain, each tap's fdm_gd <= 3 roundings (v * a, two fma with b); + 1
N_FDM_ADJ = 9 + 3 + 3 + 1       # wrt the unpadded field: <= 4 padded cells replicate a node, 3 more adds (fdm_fused_bwd_kernel, or the pad's own adjoint)


def corr_matrix(n, a, b):
    """identity except the two corner 2 x 1 blocks: column 0 holds (a, b) in rows 0, 1 and column n - 1 holds (b, a) in rows n - 2, n - 1"""
    c = torch.eye(n, dtype=torch.float64)
    c[0, 0] = c[n - 1, n - 1] = a
    c[1, 0] = c[n - 2, n - 1] = b
    return c


def fdm_kernels(domain_size):
    from diffnet_amd.fdm import get_deriv_kernels
    _, kx, ky, _, _, kxx, kyy, _ = get_deriv_kernels(2, "fdm", 3, domain_size)
    return {n: torch.from_numpy(np.ascontiguousarray(k, dtype=np.float32)).double() for n, k in (("x", kx), ("y", ky), ("xx", kxx), ("yy", kyy))}


def fdm64(u, cot, k, axis, a, b):
    """derivative, VJP wrt the padded field, VJP wrt the field: x-operators multiply by the nx x nx matrix from the right, y-operators by
    the transposed ny x ny matrix from the left"""
    ur = u.clone().requires_grad_(True)
    gp = F.pad(ur, (1, 1, 1, 1), mode="replicate")
    d = F.conv2d(gp, k.reshape(1, 1, 3, 3))
    d = torch.matmul(d, corr_matrix(u.shape[3], a, b)) if axis == 0 else torch.matmul(corr_matrix(u.shape[2], a, b).T, d)
    ggp, gu = torch.autograd.grad(d, [gp, ur], cot)
    return d.detach(), ggp, gu


def fdm_ref_and_mag(u, cot, k, name):
    axis, a, b = FDM_OPS[name]
    return fdm64(u.double(), cot.double(), k, axis, a, b), fdm64(u.abs().double(), cot.abs().double(), k.abs(), axis, abs(a), abs(b))


FDM_SHAPES = [(2, 2, 1), (2, 5, 2), (3, 3, 1), (3, 17, 2), (16, 33, 3), (40, 37, 2),      # ny, nx, B: extent 2 (both edges each other's
              (513, 411, 5)]                                                              # neighbour), 3 (the middle node takes both edge
#                                                                                           terms); 1 054 215 outputs: the grid-stride loops


@pytest.mark.gpu
@pytest.mark.parametrize("ny,nx,B", FDM_SHAPES, ids=[f"{a}x{b}_B{c}" for a, b, c in FDM_SHAPES])
def test_fdm_nonsquare_padded_and_fused(ny, nx, B):
    from DiffNet.DiffNetFDM import DiffNetFDM
    m = DiffNetFDM(None, domain_size=nx).to(dev())
    ks = fdm_kernels(nx)
    for name in FDM_OPS:
        assert tuple(float(v) for v in ks[name].reshape(-1)) == m._k[name]
        u, cot = rnd((B, 1, ny, nx), "fdm u", ny, nx, B, name), rnd((B, 1, ny, nx), "fdm cot", ny, nx, B, name)
        (d, ggp, gu), (Ad, Aggp, Agu) = fdm_ref_and_mag(u, cot, ks[name], name)
        cd = cot.to(dev())
        ur = u.to(dev()).requires_grad_(True)
        gp = (m.pad if len(name) == 1 else m.pad_d2)(ur)
        dp = getattr(m, "derivative_" + name)(gp)
        ggp_p, gu_p = torch.autograd.grad(dp, [gp, ur], cd)
        uf = u.to(dev()).requires_grad_(True)
        df = getattr(m, "d" + name)(uf)
        (gu_f,) = torch.autograd.grad(df, uf, cd)
        check("fdm", f"d{name} {ny}x{nx} B={B}", padded=(dp, d, Ad, N_FDM_FWD), padded_vjp_g=(ggp_p, ggp, Aggp, N_FDM_PAD_ADJ),
              padded_vjp_u=(gu_p, gu, Agu, N_FDM_ADJ), fused=(df, d, Ad, N_FDM_FWD), fused_vjp=(gu_f, gu, Agu, N_FDM_ADJ),
              fused_vs_padded=(df, dp.detach().double().cpu(), Ad, N_FDM_FWD), fused_vs_padded_vjp=(gu_f, gu_p.double().cpu(), Agu, N_FDM_ADJ))


# ---------------------------------------------------------------------------------------------
# 10. winding number
# ---------------------------------------------------------------------------------------------
# One term, from the kernel's loop body (csrc/winding.hip), relative errors in units of 2^-24:
#   dx = v.x - qx, dy = v.y - qy               1 each, relative to |dx|, |dy|
#   s = |dx| + |dy|                            a positive sum: max(1, 1) from the differences + 1 of its own      = 2
#   den = k * s                                k = 4 pi rounded to float32 (1) and the product (1)                 = 4
#   den * den * den                            the error of den enters three times (12), two products (2)         = 14
#   v_rcp_f32                                  1 ulp = 2                                                          = 16
#   fmaf(dx, v.z, dy * v.w)                    each numerator term: its difference (1), dy * v.w (1), the fma (1)  = 3, relative to |dx n_x| + |dy n_y|
#   acc = fmaf(numerator, rcp, acc)            the accumulation: one rounding per point, npts in all
# => c = 16 + 3 = 19 for the term itself and + 1 for the terms of second order: n = npts + 20, against
#    A = sum_p (|dx n_x| + |dy n_y|) / (4 pi (|dx| + |dy|))^3.
C_WINDING = 20
WINDING = [(1, 1, 3, 5), (2, 255, 7, 5), (3, 256, 16, 16), (2, 257, 17, 16), (2, 513, 40, 70)]      # B, npts, ny, nx
MIN_L1 = 1e-4


@functools.lru_cache(maxsize=None)
def winding_problem(B, npts, ny, nx):
    """points on ellipses that differ per sample, unit normals, nodes of the unit square; float64 reference, A and the smallest
    L1 distance between a point and a node"""
    from oracle.fem_oracle import winding_nodes
    th = torch.sort((rnd((B, npts), "winding", B, npts, ny, nx) + 0.5) * (2.0 * math.pi), dim=1).values
    b = torch.arange(B, dtype=torch.float32)[:, None]
    rx, ry = 0.27 + 0.031 * b, 0.21 - 0.017 * b
    pts = torch.stack([0.4937 + 0.0113 * b + rx * torch.cos(th), 0.4519 + 0.0071 * b + ry * torch.sin(th)], -1)
    nrm = torch.stack([torch.cos(th) / rx, torch.sin(th) / ry], -1)
    nrm = nrm / torch.linalg.vector_norm(nrm, dim=-1, keepdim=True)
    xx, yy = torch.meshgrid(torch.linspace(0, 1, nx), torch.linspace(0, 1, ny), indexing="xy")
    nodes = torch.stack((xx, yy), 0)                                            # (2, ny, nx)
    ref = winding_nodes(pts.double(), nrm.double(), nodes.double())             # (B, 1, nx, ny)
    d = pts.double()[:, None, None, :, :] - nodes.double().permute(2, 1, 0)[None, :, :, None, :]
    l1 = d.abs().sum(-1)
    A = ((d * nrm.double()[:, None, None, :, :]).abs().sum(-1) / (4 * math.pi * l1) ** 3).sum(-1)[:, None]
    return pts, nrm, nodes, ref, A, float(l1.min())


@pytest.mark.gpu
@pytest.mark.parametrize("B,npts,ny,nx", WINDING, ids=[f"B{a}_p{b}_{c}x{d}" for a, b, c, d in WINDING])
def test_winding_chunk_boundaries_and_output_order(B, npts, ny, nx):
    from diffnet_amd.ops import compute_winding_nodes
    pts, nrm, nodes, ref, A, _ = winding_problem(B, npts, ny, nx)
    w = compute_winding_nodes(pts.to(dev()).unsqueeze(1), nrm.to(dev()).unsqueeze(1), torch.zeros(B, 1, npts, 1, device=dev()), nodes.to(dev()))
    assert tuple(w.shape) == (B, 1, nx, ny)
    check("winding", f"B={B} npts={npts} {ny}x{nx}", w=(w, ref, A, npts + C_WINDING))


# ---------------------------------------------------------------------------------------------
# CPU: the comparator has teeth, the FDM restatement reproduces the reference, the winding cases keep their distance
# ---------------------------------------------------------------------------------------------
TEETH = [(2, 3, 2, (67, 11), 1, 5),         # TILED_2D[1] at degree 2
         (1, 2, 3, (50,), 3, 3),            # STRIDES[0]: nodes without a window
         (3, 3, 1, (7, 8, 9), 2, 5)]        # STRIDES[5]


@pytest.mark.parametrize("nsd,nbf,stride,nodes,B,G", TEETH, ids=[f"nsd{c[0]}_nbf{c[1]}_s{c[2]}" for c in TEETH])
def test_bound_passes_float32_and_rejects_index_errors(nsd, nbf, stride, nodes, B, G):
    x, tab, cot, y, g, Ay, Ag = gpe_problem(nsd, nbf, stride, nodes, B, G)
    nf, na = n_fwd(nsd, nbf), n_adj(nsd, nbf, G)
    y32, g32 = gpe_pair(x, tab, cot, nsd, nbf, stride)                      # a float32 evaluation of the same formulation
    ok = check("cpu_float32", f"nsd={nsd} nbf={nbf} stride={stride}", fwd=(y32, y, Ay, nf), adj=(g32, g, Ag, na))
    swapped = tab.double().clone()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]                                 # local nodes 0 and 1 exchanged: a mirrored / transposed local index
    ys, gs = gpe_pair(x.double(), swapped, cot.double(), nsd, nbf, stride)
    shifted = torch.roll(cot.double(), 1, dims=-1)                          # the cotangent one element column off
    _, gh = gpe_pair(x.double(), tab.double(), shifted, nsd, nbf, stride)
    bad = {"swapped fwd": bound_ratio(ys, y, Ay, nf), "swapped adj": bound_ratio(gs, g, Ag, na), "shifted adj": bound_ratio(gh, g, Ag, na)}
    print("exact float64 evaluations of the wrong operator:", {k: f"{v:.3g}" for k, v in bad.items()}, "against", {k: f"{v:.3g}" for k, v in ok.items()})
    for k, v in bad.items():
        assert v > 1.0, f"{k}: the bound does not notice ({v:.3g})"


@pytest.mark.parametrize("n", [16, 33])
def test_fdm_restatement_reproduces_reference_golden(n):
    """orientation of the correction matrices: the float64 restatement against what the reference computed in float32 (its conv + dense
    matmul adds exact zeros only, so the same counts hold), all four derivatives and VJPs, before it serves non-square grids"""
    z = load(f"fdm_n{n}.npz")
    ks = fdm_kernels(n)
    for name, (axis, a, b) in FDM_OPS.items():
        np.testing.assert_array_equal(ks[name].float().numpy().reshape(1, 1, 3, 3), z["par_sobel" + name])
        c = corr_matrix(n, a, b)
        np.testing.assert_array_equal((c if axis == 0 else c.T).float().numpy()[None, None], z[("par_h_corr" if axis == 0 else "par_v_corr") + ("_d2" if len(name) == 2 else "")])
        u, cot = torch.from_numpy(z["u"]), torch.from_numpy(z["cot_" + name])
        (d, _, gu), (Ad, _, Agu) = fdm_ref_and_mag(u, cot, ks[name], name)
        check("cpu_fdm_golden", f"d{name} n={n}", d=(torch.from_numpy(z["d_" + name]), d, Ad, N_FDM_FWD), vjp=(torch.from_numpy(z["vjp_" + name]), gu, Agu, N_FDM_ADJ))
        # the transposed matrix (rows and columns of the fix-up mixed up) is far outside the bound
        conv = F.conv2d(F.pad(u.double(), (1, 1, 1, 1), mode="replicate"), ks[name].reshape(1, 1, 3, 3))
        wrong = torch.matmul(conv, c.T) if axis == 0 else torch.matmul(c, conv)
        assert bound_ratio(wrong, d, Ad, N_FDM_FWD) > 1.0, name


@pytest.mark.parametrize("B,npts,ny,nx", WINDING, ids=[f"B{a}_p{b}_{c}x{d}" for a, b, c, d in WINDING])
def test_winding_cases_keep_points_off_the_nodes(B, npts, ny, nx):
    from oracle.fem_oracle import winding_nodes
    pts, nrm, nodes, ref, A, l1min = winding_problem(B, npts, ny, nx)
    print(f"smallest L1 distance point - node: {l1min:.3g}")
    assert l1min >= MIN_L1
    assert torch.allclose(torch.linalg.vector_norm(nrm, dim=-1), torch.ones(B, npts), atol=1e-6)
    # the reference's own float32 evaluation (a division and a power in place of v_rcp_f32 and two products) is within the same bound
    check("cpu_float32", f"winding B={B} npts={npts} {ny}x{nx}", w=(winding_nodes(pts, nrm, nodes), ref, A, npts + C_WINDING))
    if nx != ny:                                     # ... and the (Nx, Ny) output order is part of the check
        assert ref.shape == (B, 1, nx, ny)
