"""CPU checks of multigrid on meshes that need not be nested (mg_coarsening="general": diffnet_amd/solve.py, dn_poisson_mg_transfer in
csrc/poisson_mg_general.hip): the level rule, the option's errors, the per-axis tables and their bound of 4 children, the C ABI and its
validation before any launch, and the float64 restatement of tests/mg_general_ref.py that the GPU tests measure against -- P sums to 1
and reproduces linear functions, the V-cycle is symmetric positive definite, the iteration count does not grow with the mesh."""
import ctypes as C

import numpy as np
import pytest

import mg_general_ref as gr
import mg_ref
import solve_ref as sr
from test_mg_host import box_image
from test_solve_host import geometry
from test_stokes_host import header_struct

GROWTH_MARGIN = 2                                              # as tests/test_gpu_multigrid.py


# ---------------------------------------------------------------------------------------------
# the levels
# ---------------------------------------------------------------------------------------------
POW2 = [(512, 512), (257, 257), (129, 129), (65, 65), (33, 33), (17, 17), (9, 9), (5, 5), (3, 3)]


@pytest.mark.parametrize("sizes, shapes", [
    ((8, 8), [(8, 8), (5, 5), (3, 3)]),
    ((16, 16), [(16, 16), (9, 9), (5, 5), (3, 3)]),
    ((50, 50), [(n, n) for n in (50, 26, 14, 8, 5, 3)]),
    ((12, 7), [(7, 12), (4, 7), (3, 4)]),
    ((6, 7, 10), [(10, 7, 6), (6, 4, 4), (4, 3, 3)]),
    ((9, 4), [(4, 9), (3, 5)]),
    ((512, 512), POW2),
])
def test_general_levels(sizes, shapes):
    from diffnet_amd import solve
    g = geometry(sizes)
    lv = solve.multigrid_levels(g, coarsening="general")
    assert [s for s, _ in lv] == shapes                        # node shapes in memory order, as geom.node_shape
    assert gr.level_shapes(g.node_shape) == shapes
    for shape, hs in lv:                                       # every level covers the same box
        for h, n, h0, n0 in zip(hs, shape[::-1], g.hs, g.sizes):
            assert abs(h * (n - 1) - h0 * (n0 - 1)) <= 1e-15 * h0 * (n0 - 1)
        assert np.allclose(gr.level_geometry(g, shape).hs, hs, rtol=1e-15, atol=0)
    assert solve.multigrid_levels(g, 2, "general") == lv[:2] and solve.multigrid_levels(g, max_levels=1, coarsening="general") == lv[:1]


@pytest.mark.parametrize("sizes", [(129, 129), (13, 9)])
def test_a_nested_mesh_gets_the_same_levels_under_both_rules(sizes):
    from diffnet_amd import solve
    g = geometry(sizes)
    assert solve.multigrid_levels(g, coarsening="general") == solve.multigrid_levels(g) == solve.multigrid_levels(g, coarsening="nested")
    assert len(solve.multigrid_levels(g)) >= 3


def test_the_default_rule_is_unchanged():
    from diffnet_amd import solve
    for sizes in ((8, 8), (512, 512)):
        assert len(solve.multigrid_levels(geometry(sizes))) == 1


def test_option_errors():
    from diffnet_amd import solve
    from diffnet_amd._lib import DiffNetHipError
    g = geometry((8, 8))
    with pytest.raises(ValueError, match="mg_coarsening"):
        solve.PoissonSolver(g, 1, precondition="multigrid", mg_coarsening="bogus")
    with pytest.raises(ValueError, match="mg_coarsening"):
        solve.poisson_solve(g, precondition="multigrid", mg_coarsening="bogus")
    with pytest.raises(ValueError, match="mg_coarsening"):
        solve.multigrid_levels(g, coarsening="bogus")
    for sizes in ((9, 3), (3, 8, 8)):                          # an axis of 2 elements
        with pytest.raises(DiffNetHipError, match="cannot be coarsened"):
            solve.PoissonSolver(geometry(sizes), 1, precondition="multigrid", mg_coarsening="general")
    with pytest.raises(DiffNetHipError, match="cannot be coarsened"):
        solve.PoissonSolver(g, 1, precondition="multigrid", mg_coarsening="general", mg_max_levels=1)
    with pytest.raises(DiffNetHipError, match=r"cannot be coarsened.*k 2\^\(L-1\) \+ 1"):      # the default still refuses 8^2
        solve.PoissonSolver(g, 1, precondition="multigrid")


# ---------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [4, 5, 6, 7, 8, 9, 16, 23, 50, 128, 130, 259, 512])
def test_axis_tables_are_the_rows_and_columns_of_one_float32_matrix(nf):
    from diffnet_amd import ops
    nc = nf // 2 + 1
    assert nc == -(-(nf - 1) // 2) + 1
    parents, children = ops.mg_axis_tables(nf, nc)
    assert parents.dtype.itemsize == 16 and children.dtype.itemsize == 32 and len(parents) == nf and len(children) == nc
    P = ops.mg_axis_matrix(parents, nc)
    assert P.dtype == np.float32 and np.array_equal(P.astype(np.float64), gr.prolong_1d(nf, nc, rounded=True))
    assert np.all(parents["j"] >= 0) and np.all(parents["j"] <= nc - 2)
    Q = np.zeros_like(P)                                       # the children table, put back into a matrix
    for j, c in enumerate(children):
        assert 1 <= c["count"] <= 4 and 0 <= c["first"] and c["first"] + c["count"] <= nf
        assert not c["w"][c["count"]:].any() and np.all(c["w"][: c["count"]] != 0)
        Q[c["first"]: c["first"] + c["count"], j] = c["w"][: c["count"]]
    assert np.array_equal(P, Q), "RESTRICT reads the transpose of what PROLONG reads, bit for bit"
    if nf % 2:                                                 # a nested axis: the weights of dn_poisson_mg
        assert np.array_equal(P.astype(np.float64), mg_ref.prolong_1d(nc))
    with pytest.raises(ValueError):
        ops.mg_axis_tables(nf, nc + 1)
    with pytest.raises(ValueError):
        ops.mg_axis_tables(3, 2)


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_transfer_abi_header_binding_and_library_agree():
    from diffnet_amd import _lib, build, ops
    build.build(verbose=False)
    h = _lib.lib()
    header = open(_lib.HERE + "/../include/diffnet_hip.h").read()
    assert hasattr(h, "dn_poisson_mg_transfer") and "dn_poisson_mg_transfer" in _lib.SYMBOLS and "dn_poisson_mg_transfer(" in header
    assert "poisson_mg_general.hip" in build.SOURCES
    for cls, name in ((_lib.DnPoissonMgTransferArgs, "dn_poisson_mg_transfer_args"), (_lib.DnMgParent, "dn_mg_parent"),
                      (_lib.DnMgChildren, "dn_mg_children")):
        got = [(n, getattr(t, "_length_", 1)) for n, t in cls._fields_]
        assert got == header_struct(name), name
    T = _lib.DnPoissonMgTransferArgs
    assert C.sizeof(T) == 136 and T.x.offset == 40 and T.mask_batched.offset == 80 and T.parents.offset == 88 and T.children.offset == 112
    assert C.sizeof(_lib.DnMgParent) == 16 == np.dtype(ops.MG_PARENT_DTYPE).itemsize
    assert C.sizeof(_lib.DnMgChildren) == 32 == np.dtype(ops.MG_CHILDREN_DTYPE).itemsize and _lib.DnMgChildren.w.offset == 16
    assert [n for n, *_ in ops.MG_PARENT_DTYPE] == [n for n, _ in _lib.DnMgParent._fields_]
    assert [n for n, *_ in ops.MG_CHILDREN_DTYPE] == [n for n, _ in _lib.DnMgChildren._fields_]
    # the existing entry is as it was
    assert C.sizeof(_lib.DnPoissonMgArgs) == 104 and _lib.DnPoissonMgArgs.c.offset == 80


def test_transfer_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    fn = _lib.lib().dn_poisson_mg_transfer
    assert fn(None, None) == -1

    def args(op, nsd=2, fine=(16, 7, 1), coarse=(9, 4, 1)):
        a = _lib.DnPoissonMgTransferArgs()
        a.op, a.nsd, a.batch = op, nsd, 2
        for d in range(3):
            a.fine[d], a.coarse[d] = fine[d], coarse[d]
            a.parents[d], a.children[d] = 65536 * (d + 1), 65536 * (d + 4)
        a.x, a.b, a.q, a.c, a.mask = 1024, 2048, 4096, 16384, 32768
        return a

    for op in (-1, _lib.MG_SMOOTH, _lib.MG_SMOOTH0, 4):
        assert fn(C.byref(args(op)), None) == -1
    for op, members in ((_lib.MG_RESTRICT, "b q c"), (_lib.MG_PROLONG, "x c")):
        for mname in members.split():
            a = args(op)
            setattr(a, mname, None)
            assert fn(C.byref(a), None) == -1, (op, mname)
            a = args(op)
            setattr(a, mname, getattr(a, mname) + 4)           # off 16 bytes
            assert fn(C.byref(a), None) == -1, (op, mname)
        for table in ("parents", "children"):
            for d in (0, 1):
                a = args(op)
                getattr(a, table)[d] = None
                assert fn(C.byref(a), None) == -1, (op, table, d)
                a = args(op)
                getattr(a, table)[d] += 8
                assert fn(C.byref(a), None) == -1, (op, table, d)
        # a coarse extent other than ceil((nf - 1) / 2) + 1; an axis of 3 nodes
        for fine, coarse in (((16, 7, 1), (8, 4, 1)), ((16, 7, 1), (9, 5, 1)), ((16, 7, 1), (9, 3, 1)), ((16, 3, 1), (9, 2, 1)), ((3, 7, 1), (2, 4, 1))):
            assert fn(C.byref(args(op, 2, fine, coarse)), None) == -1, (op, fine, coarse)
        assert fn(C.byref(args(op, 3, (16, 7, 6), (9, 4, 3))), None) == -1
        assert fn(C.byref(args(op, 3, (1024, 1024, 1024), (513, 513, 513))), None) == -1        # 2^30 nodes
        for field, bad in (("nsd", 1), ("nsd", 4), ("batch", 0), ("batch", 65536), ("mask_batched", 2), ("mask_batched", -1)):
            a = args(op)
            setattr(a, field, bad)
            assert fn(C.byref(a), None) == -1, field


# ---------------------------------------------------------------------------------------------
# the float64 restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [4, 5, 6, 7, 8, 9, 12, 23, 50])
def test_interpolation_rows_sum_to_one_and_reproduce_linear_functions(nf):
    nc = nf // 2 + 1
    P = gr.prolong_1d(nf, nc)
    assert P.shape == (nf, nc) and np.max(np.abs(P.sum(1) - 1)) <= 1e-15 and np.all(P >= 0) and np.all((P != 0).sum(1) <= 2)
    lin = lambda n: 0.3 + 2.0 * np.linspace(0, 1, n)
    assert np.max(np.abs(P @ lin(nc) - lin(nf))) <= 1e-14
    assert np.all((P != 0).sum(0) <= 4), "a coarse node receives from at most 4 fine nodes"
    assert np.max(np.abs(gr.prolong_1d(nf, nc, rounded=True) - P)) <= 2.0 ** -24
    R = gr.interp_1d(nf, nc)                                   # the other way, for the coefficient
    assert np.max(np.abs(R.sum(1) - 1)) <= 1e-15 and np.max(np.abs(R @ lin(nf) - lin(nc))) <= 1e-14
    near = gr.nearest_1d(nf, nc)
    assert near[0] == 0 and near[-1] == nf - 1 and np.all(np.diff(near) >= 1)
    if nf % 2:
        assert np.array_equal(P, mg_ref.prolong_1d(nc)) and np.array_equal(near, np.arange(nc) * 2)
        assert np.array_equal(R, np.eye(nf)[::2])


def test_multilinear_fields_are_interpolated_exactly_in_2d_and_3d():
    for fine in ((7, 12), (10, 7, 6)):
        coarse = tuple(n // 2 + 1 for n in fine)
        P = gr.prolongation(fine, coarse)
        field = lambda shp: sum((d + 1.5) * g / (n - 1) for d, (g, n) in enumerate(zip(np.indices(shp), shp))).ravel()
        assert P.shape == (np.prod(fine), np.prod(coarse)) and np.max(np.abs(P @ field(coarse) - field(fine))) <= 1e-13


def test_on_a_nested_mesh_the_general_hierarchy_is_the_nested_one():
    g = geometry((13, 9))
    nu = np.random.default_rng(0).uniform(0.5, 1.5, g.node_shape)
    box = box_image(tuple(g.node_shape))
    for a, b in zip(gr.hierarchy(g, nu, box, 0.7), mg_ref.hierarchy(g, nu, box, 0.7)):
        assert a["shape"] == b["shape"] and np.array_equal(a["fixed"], b["fixed"])
        assert np.allclose(a["K"], b["K"], rtol=1e-13, atol=1e-13 * np.max(np.abs(b["K"])))
        assert (a["P"] is None and b["P"] is None) or np.array_equal(a["P"], b["P"])


def problems(sizes):
    """(name, nu, fixed) on a mesh: random nu, contrast-300 nu, and an immersed Dirichlet disk beside the box faces."""
    g = geometry(sizes)
    shp = tuple(g.node_shape)
    rng = np.random.default_rng(len(sizes))
    box = box_image(shp)
    grids = np.indices(shp)
    centre = [(s - 1) * 0.5 + 0.3 for s in shp]
    disk = sum((grids[d] - centre[d]) ** 2 for d in range(len(shp))) <= (0.22 * min(shp)) ** 2
    assert disk.any()
    return g, [("random", rng.uniform(0.5, 1.5, shp), box), ("contrast300", np.exp(rng.uniform(0, np.log(300.0), shp)), box),
               ("disk", rng.uniform(0.5, 1.5, shp), box | disk)]


@pytest.mark.parametrize("sizes", [(8, 8), (12, 7), (6, 6, 6)])
@pytest.mark.parametrize("rounded", [False, True], ids=["exact-weights", "float32-weights"])
def test_the_general_vcycle_is_symmetric_positive_definite(sizes, rounded):
    from diffnet_amd import solve
    g, probs = problems(sizes)
    omega = solve.default_mg_omega(g)
    jac = float(np.prod([0.5 * h for h in g.hs]))
    for name, nu, fixed in probs:
        lv = gr.hierarchy(g, nu, fixed, jac, rounded=rounded)
        assert len(lv) >= 2
        free = ~fixed.ravel()
        for sweeps, coarse in ((1, 4), (2, 1)):
            M = gr.preconditioner_matrix(lv, sweeps=sweeps, omega=omega, coarse_sweeps=coarse)
            assert not M[~free].any(), "z is zero on the Dirichlet nodes"
            Mf = M[np.ix_(free, free)]
            scale = np.max(np.abs(Mf))
            print(f"{sizes} {name} sweeps {sweeps}: |M - M^T| = {np.max(np.abs(Mf - Mf.T)) / scale:.2e} max|M|")
            assert np.max(np.abs(Mf - Mf.T)) <= 1e-12 * scale, name
            ev = np.linalg.eigvalsh(0.5 * (Mf + Mf.T))
            assert ev[0] > 1e-6 * ev[-1], (name, ev[0], ev[-1])


COUNTS = {}


def reference_count(n):
    """(geom, nu, f, float64 PCG iterations, Jacobi iterations) at n^2, random nu in [0.5, 1.5], box faces, tol 1e-5; computed once and
    shared with tests/test_gpu_multigrid_general.py."""
    from diffnet_amd import solve
    if n not in COUNTS:
        g = geometry((n, n))
        rng = np.random.default_rng(n)
        nu, f = rng.uniform(0.5, 1.5, g.node_shape), rng.standard_normal(g.node_shape)
        box = box_image(tuple(g.node_shape))
        K, b = sr.dense_system(g, nu, f)
        _, info = gr.pcg(K, b, [(box, 0.0)], levels=gr.hierarchy(g, nu, box), tol=1e-5, omega=solve.default_mg_omega(g))
        assert info["converged"]
        COUNTS[n] = (g, nu, f, info["iterations"])
    return COUNTS[n]


def test_reference_iteration_count_is_mesh_independent():
    its = {n: reference_count(n)[3] for n in (16, 32, 64)}
    print("float64 restatement iterations, general coarsening", its)
    assert its[64] <= its[16] + GROWTH_MARGIN


@pytest.mark.parametrize("sizes", [(16, 16), (23, 16), (8, 8, 8)])
def test_pcg_with_the_general_vcycle_reproduces_the_dense_solve(sizes):
    from diffnet_amd import solve
    g, probs = problems(sizes)
    omega = solve.default_mg_omega(g)
    rng = np.random.default_rng(7)
    name, nu, fixed = probs[2]
    f, val = rng.standard_normal(g.node_shape), rng.standard_normal(g.node_shape)
    K, b = sr.dense_system(g, nu, f)
    cond = [(fixed, val)]
    u = sr.dense_solve(K, b, cond)
    x, info = gr.pcg(K, b, cond, levels=gr.hierarchy(g, nu, fixed), tol=1e-10, omega=omega)
    xj, ij = sr.cg_restated(K, b, cond, tol=1e-10)
    assert info["converged"] and np.max(np.abs(x - u)) <= 1e-8 * np.max(np.abs(u))
    assert info["iterations"] < ij["iterations"], (info["iterations"], ij["iterations"])
