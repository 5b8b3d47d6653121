"""CPU checks of the multigrid preconditioner (dn_poisson_mg: csrc/poisson_mg.hip; dn_poisson_pcg: csrc/poisson_cg.hip;
diffnet_amd/solve.py): the level lists, the C ABI and its binding, argument validation before any launch, and the float64 restatement
of tests/mg_ref.py that the GPU tests measure against -- rediscretisation equals the Galerkin product for a constant coefficient, the
V-cycle is a symmetric positive definite operator with the default damping, and PCG with it reproduces the dense solve."""
import ctypes as C

import numpy as np
import pytest

import mg_ref
import solve_ref as sr
from test_solve_host import geometry
from test_stokes_host import header_struct


def box_image(shp):
    box = np.zeros(shp, bool)
    for ax in range(len(shp)):
        idx = [slice(None)] * len(shp)
        idx[ax] = 0; box[tuple(idx)] = True
        idx[ax] = -1; box[tuple(idx)] = True
    return box


# ---------------------------------------------------------------------------------------------
# the levels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes, shapes", [
    ((9, 9), [(9, 9), (5, 5), (3, 3)]),
    ((17, 9), [(9, 17), (5, 9), (3, 5)]),
    ((13, 9), [(9, 13), (5, 7), (3, 4)]),                      # 12 -> 6 -> 3 elements: the odd count stops it at 4 nodes (k = 3)
    ((9, 5, 17), [(17, 5, 9), (9, 3, 5)]),                     # the 4-element axis may be halved once
    ((129, 129), [(129, 129), (65, 65), (33, 33), (17, 17), (9, 9), (5, 5), (3, 3)]),
])
def test_multigrid_levels(sizes, shapes):
    from diffnet_amd import solve
    g = geometry(sizes)
    lv = solve.multigrid_levels(g)
    assert [s for s, _ in lv] == shapes                        # node shapes in memory order, as geom.node_shape
    assert [s for s in mg_ref.level_shapes(g.node_shape)] == shapes
    for l, (_, hs) in enumerate(lv):
        assert hs == tuple(h * 2 ** l for h in g.hs)
    assert solve.multigrid_levels(g, max_levels=2) == lv[:2] and solve.multigrid_levels(g, max_levels=1) == lv[:1]


@pytest.mark.parametrize("sizes", [(8, 8), (512, 512), (9, 4)])
def test_meshes_that_cannot_be_coarsened_raise_before_anything_touches_a_device(sizes):
    from diffnet_amd import solve
    from diffnet_amd._lib import DiffNetHipError
    g = geometry(sizes)
    assert len(solve.multigrid_levels(g)) == 1
    with pytest.raises(DiffNetHipError, match=r"k 2\^\(L-1\) \+ 1"):
        solve.PoissonSolver(g, 1, precondition="multigrid")
    with pytest.raises(DiffNetHipError, match=r"k 2\^\(L-1\) \+ 1"):
        solve.poisson_solve(g, precondition="multigrid")
    with pytest.raises(DiffNetHipError, match="cannot be coarsened"):
        solve.PoissonSolver(geometry((9, 9)), 1, precondition="multigrid", mg_max_levels=1)
    with pytest.raises(ValueError, match="precondition"):
        solve.PoissonSolver(g, 1, precondition="ilu")


def test_default_omega_from_the_element_matrix():
    from diffnet_amd import solve
    for sizes, lengths, lam in (((9, 9), None, 1.5), ((9, 9, 9), None, 1.5), ((17, 9), None, 2.4), ((17, 9), (1.0, 2.0), 48 / 17),
                                ((9, 5, 17), None, 24 / 7), ((9, 9, 9), (1.0, 1.0, 4.0), 24 / 11)):
        g = geometry(sizes, lengths=lengths)
        assert abs(solve.element_lambda_max(g) - lam) < 1e-12, (sizes, lengths)
        assert abs(solve.default_mg_omega(g) * lam - 4 / 3) < 1e-12
        # the element value bounds the assembled constant-coefficient operator's, and is attained without Dirichlet nodes
        K = sr.dense_stiffness(g)
        d = np.diag(K)
        top = np.linalg.eigvalsh(K / np.sqrt(np.outer(d, d)))[-1]
        assert top <= lam + 1e-12 and top >= lam - 1e-9


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_multigrid_abi_header_binding_and_library_agree():
    from diffnet_amd import _lib, build, ops
    build.build(verbose=False)
    h = _lib.lib()
    header = open(_lib.HERE + "/../include/diffnet_hip.h").read()
    for s in ("dn_poisson_mg", "dn_poisson_pcg"):
        assert hasattr(h, s) and s in _lib.SYMBOLS and s + "(" in header, s
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    assert "poisson_mg.hip" in build.SOURCES
    for cls, name in ((_lib.DnPoissonMgArgs, "dn_poisson_mg_args"), (_lib.DnPoissonPcgArgs, "dn_poisson_pcg_args")):
        got = [(n, getattr(t, "_length_", 1)) for n, t in cls._fields_]
        assert got == header_struct(name), name
    assert C.sizeof(_lib.DnPoissonPcgArgs) == 88 and _lib.DnPoissonPcgArgs.z.offset == 48 and _lib.DnPoissonPcgArgs.state.offset == 64
    assert C.sizeof(_lib.DnPoissonMgArgs) == 104 and _lib.DnPoissonMgArgs.x.offset == 40 and _lib.DnPoissonMgArgs.c.offset == 80
    assert (_lib.PCG_RESID0, _lib.PCG_UPDATE, _lib.PCG_RZ, _lib.PCG_DIRECTION) == (0, 1, 2, 3)
    assert (_lib.MG_RESTRICT, _lib.MG_PROLONG, _lib.MG_SMOOTH, _lib.MG_SMOOTH0) == (0, 1, 2, 3)
    for name, val in (("DN_PCG_RESID0", 0), ("DN_PCG_UPDATE", 1), ("DN_PCG_RZ", 2), ("DN_PCG_DIRECTION", 3),
                      ("DN_MG_RESTRICT", 0), ("DN_MG_PROLONG", 1), ("DN_MG_SMOOTH", 2), ("DN_MG_SMOOTH0", 3)):
        assert f"{name} = {val}" in header
    assert set(ops.PCG_PHASES.values()) == {0, 1, 2, 3} and set(ops.MG_OPS.values()) == {0, 1, 2, 3}
    # the existing entry is as it was
    assert C.sizeof(_lib.DnPoissonCgArgs) == 96 and "DN_CG_DIRECTION = 3" in header


def test_pcg_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    fn = h.dn_poisson_pcg
    assert fn(None, None) == -1
    n, B = 289, 3
    need = h.dn_poisson_cg_workspace_bytes(n, B)

    def args(phase):
        a = _lib.DnPoissonPcgArgs()
        a.phase, a.batch, a.n = phase, B, n
        a.x, a.r, a.p, a.q, a.z, a.state, a.workspace, a.workspace_bytes = 1024, 2048, 4096, 8192, 16384, 32768, 65536, need
        return a

    for ph in (-1, 4, 17):
        assert fn(C.byref(args(ph)), None) == -1
    for ph, members in ((_lib.PCG_RESID0, "r q state workspace"), (_lib.PCG_UPDATE, "x r p q state workspace"),
                        (_lib.PCG_RZ, "r z state workspace"), (_lib.PCG_DIRECTION, "p z state")):
        for mname in members.split():                          # a NULL array the phase uses
            a = args(ph)
            setattr(a, mname, None)
            assert fn(C.byref(a), None) == -1, (ph, mname)
    a = args(_lib.PCG_RZ)
    a.workspace_bytes = need - 1
    assert fn(C.byref(a), None) == -1
    a = args(_lib.PCG_RZ)
    a.z = 16388                                                # an array base off 16 bytes
    assert fn(C.byref(a), None) == -1
    for field, bad, rc in (("n", 0, -1), ("batch", 0, -1), ("batch", 70000, -1), ("n", 1 << 30, -2), ("tol", -1.0, -1), ("atol", float("nan"), -1)):
        a = args(_lib.PCG_UPDATE)
        setattr(a, field, bad)
        assert fn(C.byref(a), None) == rc, field


def test_mg_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    fn = _lib.lib().dn_poisson_mg
    assert fn(None, None) == -1

    def args(op, nsd=2, fine=(17, 9, 1), coarse=(9, 5, 1)):
        a = _lib.DnPoissonMgArgs()
        a.op, a.nsd, a.batch = op, nsd, 2
        for d in range(3):
            a.fine[d], a.coarse[d] = fine[d], coarse[d]
        a.x, a.b, a.q, a.dinv, a.c, a.mask, a.omega = 1024, 2048, 4096, 8192, 16384, 32768, 0.8
        return a

    for op in (-1, 4):
        assert fn(C.byref(args(op)), None) == -1
    for op, members in ((_lib.MG_RESTRICT, "b q c"), (_lib.MG_PROLONG, "x c"), (_lib.MG_SMOOTH, "x b q dinv"), (_lib.MG_SMOOTH0, "x b dinv")):
        for mname in members.split():
            a = args(op)
            setattr(a, mname, None)
            assert fn(C.byref(a), None) == -1, (op, mname)
            a = args(op)
            setattr(a, mname, getattr(a, mname) + 4)           # off 16 bytes
            assert fn(C.byref(a), None) == -1, (op, mname)
    for op in (_lib.MG_RESTRICT, _lib.MG_PROLONG):
        for fine, coarse in (((17, 9, 1), (9, 4, 1)), ((17, 9, 1), (8, 5, 1)), ((16, 9, 1), (8, 5, 1)), ((17, 2, 1), (9, 1, 1))):
            assert fn(C.byref(args(op, 2, fine, coarse)), None) == -1, (op, fine, coarse)       # a coarse shape that does not match
        assert fn(C.byref(args(op, 3, (17, 9, 5), (9, 5, 2))), None) == -1
    for field, bad, rc in (("nsd", 1, -1), ("nsd", 4, -1), ("batch", 0, -1), ("batch", 65536, -1), ("dinv_batched", 2, -1), ("mask_batched", -1, -1),
                           ("omega", float("nan"), -1)):
        a = args(_lib.MG_SMOOTH)
        setattr(a, field, bad)
        assert fn(C.byref(a), None) == rc, field
    assert fn(C.byref(args(_lib.MG_SMOOTH, 2, (1, 9, 1))), None) == -1
    assert fn(C.byref(args(_lib.MG_SMOOTH, 3, (1024, 1024, 1024), (1, 1, 1))), None) == -2      # 2^30 nodes


# ---------------------------------------------------------------------------------------------
# the float64 restatement
# ---------------------------------------------------------------------------------------------
def test_prolongation_matrices():
    P = mg_ref.prolong_1d(3)
    assert np.array_equal(P, [[1, 0, 0], [.5, .5, 0], [0, 1, 0], [0, .5, .5], [0, 0, 1]])
    P2 = mg_ref.prolongation((3, 5))                           # (ny, nx) coarse -> (5, 9) fine
    assert P2.shape == (45, 15) and np.allclose(P2.sum(1), 1.0)
    x = np.linspace(0, 1, 9)[None, :] + 3 * np.linspace(0, 1, 5)[:, None]      # a bilinear field is interpolated exactly
    assert np.allclose(P2 @ x[::2, ::2].ravel(), x.ravel(), atol=1e-15)
    # restriction weights per axis 1/2, 1, 1/2, and nothing renormalised at the faces
    assert np.array_equal(P.T.sum(1), [1.5, 2.0, 1.5])


@pytest.mark.parametrize("sizes, lengths", [((9, 9), None), ((17, 9), (1.0, 3.0)), ((5, 5, 5), None), ((9, 5, 5), (2.0, 1.0, 0.5))])
def test_rediscretisation_is_the_galerkin_product_for_a_constant_coefficient(sizes, lengths):
    g = geometry(sizes, lengths=lengths)
    jac = float(np.prod([0.5 * h for h in g.hs]))
    for nu in (None, 2.5):
        lv = mg_ref.hierarchy(g, None if nu is None else np.full(g.node_shape, nu), None, jac)
        assert len(lv) >= 2
        for fine, coarse in zip(lv, lv[1:]):
            P = fine["P"]
            gal = P.T @ fine["K"] @ P
            assert np.max(np.abs(gal - coarse["K"])) <= 1e-12 * np.max(np.abs(gal))
    # wscale of level l is jac 2^(nsd l): the level's own Jacobian
    g1 = mg_ref.level_geometry(g, 1)
    assert abs(float(np.prod([0.5 * h for h in g1.hs])) - jac * 2 ** g.nsd) <= 1e-15 * jac * 2 ** g.nsd
    assert np.max(np.abs(lv[1]["K"] - sr.dense_stiffness(g1, np.full(g1.node_shape, 2.5), jac * 2 ** g.nsd))) == 0


def problems(sizes):
    """(name, nu, fixed) on a mesh: random nu, contrast-300 nu, and an immersed Dirichlet disk beside the box faces."""
    g = geometry(sizes)
    shp = tuple(g.node_shape)
    rng = np.random.default_rng(len(sizes))
    box = box_image(shp)
    grids = np.indices(shp)
    centre = [(s - 1) * 0.5 + 0.3 for s in shp]
    disk = sum((grids[d] - centre[d]) ** 2 for d in range(len(shp))) <= (0.22 * min(shp)) ** 2
    assert disk.any() and not disk[tuple(slice(None, None, 2) for _ in shp)].all()
    return g, [("random", rng.uniform(0.5, 1.5, shp), box), ("contrast300", np.exp(rng.uniform(0, np.log(300.0), shp)), box),
               ("disk", rng.uniform(0.5, 1.5, shp), box | disk)]


@pytest.mark.parametrize("sizes", [(9, 9), (5, 5, 5)])
def test_the_vcycle_is_symmetric_positive_definite_with_the_default_damping(sizes):
    from diffnet_amd import solve
    g, probs = problems(sizes)
    omega = solve.default_mg_omega(g)
    jac = float(np.prod([0.5 * h for h in g.hs]))
    for name, nu, fixed in probs:
        lv = mg_ref.hierarchy(g, nu, fixed, jac)
        free = ~fixed.ravel()
        for sweeps, coarse in ((1, 4), (2, 1)):
            M = mg_ref.preconditioner_matrix(lv, sweeps=sweeps, omega=omega, coarse_sweeps=coarse)
            assert not M[~free].any(), "z is zero on the Dirichlet nodes"
            Mf = M[np.ix_(free, free)]
            scale = np.max(np.abs(Mf))
            assert np.max(np.abs(Mf - Mf.T)) <= 1e-12 * scale, name
            ev = np.linalg.eigvalsh(0.5 * (Mf + Mf.T))
            assert ev[0] > 1e-6 * ev[-1], (name, ev[0], ev[-1])
            # and it is a preconditioner: the spectrum of M K is far narrower than that of D^-1 K
            K = lv[0]["K"][np.ix_(free, free)]
            Lc = np.linalg.cholesky(K)
            mk = np.linalg.eigvalsh(Lc.T @ Mf @ Lc)
            d = np.diag(K)
            dk = np.linalg.eigvalsh(K / np.sqrt(np.outer(d, d)))
            print(f"{sizes} {name} sweeps {sweeps}: cond(M K) = {mk[-1] / mk[0]:.2f}, cond(D^-1 K) = {dk[-1] / dk[0]:.2f}, omega lambda_max = {omega * dk[-1]:.3f}")
            assert omega * dk[-1] < 1.6, "omega lambda_max(D^-1 K) < 2 with a visible margin"
            assert mk[-1] / mk[0] < dk[-1] / dk[0]


@pytest.mark.parametrize("sizes", [(17, 9), (13, 9), (9, 9, 9)])
def test_pcg_with_the_vcycle_reproduces_the_dense_solve(sizes):
    from diffnet_amd import solve
    g, probs = problems(sizes)
    omega = solve.default_mg_omega(g)
    jac = float(np.prod([0.5 * h for h in g.hs]))
    rng = np.random.default_rng(7)
    for name, nu, fixed in probs:
        f = rng.standard_normal(g.node_shape)
        val = rng.standard_normal(g.node_shape)
        K, b = sr.dense_system(g, nu, f, None, jac)
        cond = [(fixed, val)]
        u = sr.dense_solve(K, b, cond)
        lv = mg_ref.hierarchy(g, nu, fixed, jac)
        x, info = mg_ref.pcg(K, b, cond, levels=lv, tol=1e-10, omega=omega)
        xj, ij = sr.cg_restated(K, b, cond, tol=1e-10)
        assert info["converged"] and np.max(np.abs(x - u)) <= 1e-8 * np.max(np.abs(u)), name
        assert info["iterations"] < ij["iterations"], (name, info["iterations"], ij["iterations"])
        x32, i32 = mg_ref.pcg(K, b, cond, levels=lv, tol=1e-5, omega=omega, dtype=np.float32)
        assert i32["converged"] and np.max(np.abs(x32 - u)) <= 1e-3 * np.max(np.abs(u)), name
