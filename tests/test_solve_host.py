"""CPU checks of the batched CG solve (dn_poisson_diag, dn_poisson_cg: csrc/poisson_cg.hip; diffnet_amd/solve.py): the C ABI and its
ctypes binding agree, the library validates its arguments before any launch, and the float64 reference of tests/solve_ref.py -- which
the GPU tests measure against -- is itself pinned to oracle/fem_oracle.py on golden cases and has teeth: its CG restatement
reproduces the dense solve."""
import ctypes as C

import numpy as np
import pytest
import torch

import solve_ref as sr
from conftest import GOLDEN
from oracle.fem_oracle import Oracle
from test_stokes_host import header_struct, stokes_mesh


def geometry(sizes_xyz, ngp=2, deg=1, lengths=None):
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    gx, gw = gauss_rule(ngp)
    lengths = lengths or (1.0,) * len(sizes_xyz)
    hs = tuple(L / ((s - 1) // deg) for L, s in zip(lengths, sizes_xyz))
    return FemGeometry(len(sizes_xyz), sizes_xyz, hs, deg, ngp, gx, gw)


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_solve_abi_header_binding_and_library_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    header = open(_lib.HERE + "/../include/diffnet_hip.h").read()
    for s in ("dn_poisson_diag", "dn_poisson_cg", "dn_poisson_cg_workspace_bytes"):
        assert hasattr(h, s) and s in _lib.SYMBOLS and s + "(" in header, s
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    assert "poisson_cg.hip" in build.SOURCES
    for cls, name in ((_lib.DnPoissonDiagArgs, "dn_poisson_diag_args"), (_lib.DnCgState, "dn_cg_state"), (_lib.DnPoissonCgArgs, "dn_poisson_cg_args")):
        got = [(n, getattr(t, "_length_", 1)) for n, t in cls._fields_]
        assert got == header_struct(name), name
    assert C.sizeof(_lib.DnCgState) == 64 and _lib.DnCgState.alpha.offset == 32 and _lib.DnCgState.active.offset == 40
    assert C.sizeof(_lib.DnPoissonDiagArgs) == 16 + 2 * C.sizeof(_lib.DnDirichlet) + 16        # the C layout (x86-64)
    assert C.sizeof(_lib.DnPoissonCgArgs) == 96 and _lib.DnPoissonCgArgs.state.offset == 72
    assert (_lib.CG_INIT, _lib.CG_DOT, _lib.CG_UPDATE, _lib.CG_DIRECTION, _lib.CG_BREAKDOWN) == (0, 1, 2, 3, 1)
    for name, val in (("DN_CG_INIT", 0), ("DN_CG_DOT", 1), ("DN_CG_UPDATE", 2), ("DN_CG_DIRECTION", 3), ("DN_CG_BREAKDOWN", 1)):
        assert f"{name} = {val}" in header
    from diffnet_amd import ops
    assert np.dtype(ops.CG_STATE_DTYPE).itemsize == 64 and np.dtype(ops.CG_STATE_DTYPE).fields["active"][1] == 40


def test_diag_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    fn = h.dn_poisson_diag
    m = stokes_mesh()
    assert fn(None, None, None) == -1 and fn(C.byref(m), None, None) == -1
    a = _lib.DnPoissonDiagArgs()
    assert fn(C.byref(m), C.byref(a), None) == -1          # NULL output
    a.dinv = 64
    for kind in (_lib.MASK_BITS, _lib.MASK_BOX):           # compact masks are expanded by the caller
        a.bc[0].mask_kind = kind
        assert fn(C.byref(m), C.byref(a), None) == -2
    a.bc[0].mask_kind = 7
    assert fn(C.byref(m), C.byref(a), None) == -1
    a.bc[0].mask_kind = _lib.MASK_F32
    a.unit = 2
    assert fn(C.byref(m), C.byref(a), None) == -1
    a.unit = 0
    for field, bad, rc in (("degree", 2, -2), ("degree", 3, -2), ("ngp", 5, -2), ("ngp", 1, -2), ("nsd", 1, -2), ("nx", 1, -1), ("batch", 0, -1)):
        mm = stokes_mesh()
        setattr(mm, field, bad)
        assert fn(C.byref(mm), C.byref(a), None) == rc, field
    m3 = geometry((5, 5, 5), ngp=3, deg=2).mesh_struct(1)      # 3-D Q2
    assert fn(C.byref(m3), C.byref(a), None) == -2


def test_cg_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    fn, wsb = h.dn_poisson_cg, h.dn_poisson_cg_workspace_bytes
    assert fn(None, None) == -1
    n, B = 289, 3
    need = wsb(n, B)
    assert need == (64 * 65 + 2 * 8 * 1) * B               # per sample: its arrival counters + two arrays of one partial
    assert wsb(70001, 2) == (64 * 65 + 2 * 8 * 69) * 2 and wsb(0, 1) == 0 and wsb(10, 0) == 0 and wsb(1 << 30, 1) == 0
    assert wsb(1024 * 2048 + 1, 1) == 64 * 65 + 2 * 8 * 1025     # past 2048 workgroups a sample the chunk doubles

    def args(phase):
        a = _lib.DnPoissonCgArgs()
        a.phase, a.batch, a.n = phase, B, n
        a.x, a.r, a.p, a.q, a.dinv, a.state, a.workspace, a.workspace_bytes = 1024, 2048, 4096, 8192, 16384, 32768, 65536, need
        return a

    for ph in (-1, 4, 17):                                 # an unknown phase
        assert fn(C.byref(args(ph)), None) == -1
    for ph, members in ((_lib.CG_INIT, "rpq dinv state workspace"), (_lib.CG_DOT, "p q state workspace"),
                        (_lib.CG_UPDATE, "x r p q dinv state workspace"), (_lib.CG_DIRECTION, "r p dinv state")):
        for mname in members.replace("rpq", "r p q").split():          # a NULL array the phase uses
            a = args(ph)
            setattr(a, mname, None)
            assert fn(C.byref(a), None) == -1, (ph, mname)
    a = args(_lib.CG_DOT)
    a.workspace_bytes = need - 1                           # a workspace that is too small
    assert fn(C.byref(a), None) == -1
    a = args(_lib.CG_UPDATE)
    a.x = 1028                                             # an array base off 16 bytes
    assert fn(C.byref(a), None) == -1
    for field, bad, rc in (("n", 0, -1), ("batch", 0, -1), ("batch", 70000, -1), ("n", 1 << 30, -2), ("dinv_batched", 2, -1), ("tol", -1.0, -1),
                           ("atol", float("nan"), -1)):
        a = args(_lib.CG_UPDATE)
        setattr(a, field, bad)
        assert fn(C.byref(a), None) == rc, field


def test_solver_refuses_degree_two_and_cpu_use():
    from diffnet_amd import DiffNet2DFEM, solve
    from diffnet_amd._lib import DiffNetHipError
    m2 = DiffNet2DFEM(None, domain_size=9, fem_basis_deg=2)
    with pytest.raises(DiffNetHipError, match="Q1"):
        solve.poisson_solve(m2.geom)
    with pytest.raises(DiffNetHipError, match="Q1"):
        m2.solve()
    m = DiffNet2DFEM(None, domain_size=9)
    assert hasattr(m, "solve")
    v = torch.zeros((1, 1, 9, 9), requires_grad=True)
    with pytest.raises(DiffNetHipError, match="no gradient"):
        solve.poisson_solve(m.geom, dirichlet=[(torch.ones((1, 1, 9, 9)), v)])


# ---------------------------------------------------------------------------------------------
# the reference is the oracle's operator
# ---------------------------------------------------------------------------------------------
def exact_tables(o):
    """The oracle's Q1 value and first-derivative tables and weights again, by its own rule and basis functions and in its own
    layout, but kept in float64 (build_tables rounds each entry to float32 on store, which is all that separates it from 1e-12)."""
    from oracle.fem_oracle import basis_1d
    s = o.spec
    nsd, ng = s.nsd, s.ngp_1d
    B1 = [basis_1d(1, float(x)) for x in s.gpx_1d]
    sx = [2.0 / h for h in s.hs]
    names = ["N_gp"] + ["dN_%s_gp" % a for a in "xyz"[:nsd]]
    vals = ["Nvalues"] + ["dN_%s_values" % a for a in "xyz"[:nsd]]
    K = {n: np.zeros((s.ngp_total,) + (2,) * nsd) for n in names}
    gpw = np.zeros(s.ngp_total)
    for g, gp in enumerate(np.ndindex(*(ng,) * nsd)):              # (kg, jg, ig): x fastest
        gpw[g] = np.prod([s.gpw_1d[q] for q in gp])
        for c in np.ndindex(*(2,) * nsd):                           # (kb, jb, ib)
            val = [B1[gp[ax]][0][c[ax]] for ax in range(nsd)]
            der = [B1[gp[ax]][1][c[ax]] for ax in range(nsd)]
            K["N_gp"][(g,) + c] = np.prod(val)
            for d, a in enumerate("xyz"[:nsd]):
                ax = nsd - 1 - d                                    # x is the last memory axis
                K["dN_%s_gp" % a][(g,) + c] = der[ax] * np.prod([val[q] for q in range(nsd) if q != ax]) * sx[d]
    for kn, vn in zip(names, vals):
        new = (K[kn].reshape((s.ngp_total, 1, 1) + (2,) * nsd), np.moveaxis(K[kn].reshape(s.ngp_total, -1), 0, 1).reshape((1, 2 ** nsd, s.ngp_total) + (1,) * nsd))
        for old, nw in zip((o.t[kn], o.t[vn]), new):              # the same tables: they round to the oracle's float32 entries
            assert old.shape == nw.shape and np.array_equal(old.numpy(), nw.astype(np.float32))
        o.t[kn] = torch.from_numpy(K[kn].reshape((s.ngp_total, 1, 1) + (2,) * nsd))
        o.t[vn] = torch.from_numpy(np.moveaxis(K[kn].reshape(s.ngp_total, -1), 0, 1).reshape((1, 2 ** nsd, s.ngp_total) + (1,) * nsd).copy())
    o.t["gpw"] = o.gpw = torch.from_numpy(gpw)


@pytest.mark.parametrize("name", ["loss_e8_2d_n17", "loss_e8_3d_n9"])
def test_dense_system_reproduces_the_oracle_residual(name):
    z = np.load(f"{GOLDEN}/{name}.npz", allow_pickle=True)
    kw = eval(str(z["kwargs"]))
    o = Oracle(**kw)
    nsd, n = o.nsd, kw["domain_size"]
    tt = lambda a: torch.from_numpy(np.asarray(a)).double()
    exact_tables(o)
    inp = tt(z["inputs"])
    nu, bc2 = inp[:, 0:1], inp[:, 2:3]
    ubc, fgp, u = tt(z["u_bc"])[None, None], tt(z["f_gp"]), tt(z["u"])
    jac = (0.5 / (n - 1)) ** nsd
    R = o.residual(u, nu, f_gp=fgp, dirichlet=[(bc2, ubc)], jac=jac, zero_masks=[bc2]).numpy().ravel()
    geom = geometry((n,) * nsd)
    K, b = sr.dense_system(geom, nu=nu[0, 0].numpy(), f_gp=fgp[0].numpy(), jac=jac)
    cond = [(bc2[0, 0].numpy() > 0.5, ubc[0, 0].numpy())]
    ut = sr.substitute(u[0, 0].numpy(), cond)
    mine = np.where(sr.fixed_nodes(len(b), cond), 0.0, K @ ut - b)
    assert np.max(np.abs(mine - R)) <= 1e-12 * max(1.0, np.max(np.abs(R)))
    assert np.max(np.abs(R)) > 1e-6                        # the case exercises the operator
    # nodal forcing takes the same route: f interpolated to the Gauss points
    f = np.random.default_rng(3).standard_normal(geom.node_shape)
    Rf = o.residual(u, nu, f=tt(f)[None, None], dirichlet=[(bc2, ubc)], jac=jac, zero_masks=[bc2]).numpy().ravel()
    _, bf = sr.dense_system(geom, nu=nu[0, 0].numpy(), f=f, jac=jac)
    assert np.max(np.abs(np.where(sr.fixed_nodes(len(b), cond), 0.0, K @ ut - bf) - Rf)) <= 1e-12 * max(1.0, np.max(np.abs(Rf)))


# ---------------------------------------------------------------------------------------------
# teeth of the reference
# ---------------------------------------------------------------------------------------------
def small_case(sizes, seed, ngp=2):
    geom = geometry(sizes, ngp=ngp)
    rng = np.random.default_rng(seed)
    shp = geom.node_shape
    nu = rng.uniform(0.5, 1.5, shp)
    f = rng.standard_normal(shp) * 10
    box = np.zeros(shp, bool)
    for ax in range(len(shp)):
        idx = [slice(None)] * len(shp)
        idx[ax] = 0; box[tuple(idx)] = True
        idx[ax] = -1; box[tuple(idx)] = True
    val = rng.standard_normal(shp)
    return geom, nu, f, [(box, val)]


@pytest.mark.parametrize("sizes", [(9, 9), (5, 5, 5)])
def test_float64_cg_equals_the_dense_solve_and_float32_converges(sizes):
    geom, nu, f, cond = small_case(sizes, 11, ngp=3)
    K, b = sr.dense_system(geom, nu, f)
    assert np.max(np.abs(K - K.T)) <= 1e-12 * np.max(np.abs(K)) and np.max(np.abs(K.sum(1))) <= 1e-10 * np.max(np.abs(K))
    u = sr.dense_solve(K, b, cond)
    fx = sr.fixed_nodes(len(b), cond)
    assert np.array_equal(u[fx], cond[0][1].ravel()[fx])
    x64, i64 = sr.cg_restated(K, b, cond, tol=1e-13, dtype=np.float64)
    assert i64["converged"] and not i64["breakdown"] and 0 < i64["iterations"] <= len(b)
    assert np.max(np.abs(x64 - u)) <= 1e-10 * np.max(np.abs(u))
    x32, i32 = sr.cg_restated(K, b, cond, tol=1e-6, dtype=np.float32)
    assert i32["converged"] and i32["iterations"] <= 4 * i64["iterations"]
    err32 = np.max(np.abs(x32 - u)) / np.max(np.abs(u))          # the yardstick the GPU tests compute the same way
    assert 0 < err32 < 1e-4
    assert np.array_equal(x32[fx], cond[0][1].ravel().astype(np.float32)[fx])
    # without the preconditioner: the same solution
    xn, inn = sr.cg_restated(K, b, cond, dinv=sr.dense_dinv(K, fx, unit=True), tol=1e-13, dtype=np.float64)
    assert inn["converged"] and np.max(np.abs(xn - u)) <= 1e-10 * np.max(np.abs(u))


def test_guards_of_the_restatement():
    geom, nu, f, cond = small_case((9, 9), 5)
    K, b = sr.dense_system(geom, nu, f)
    # rr0 = 0: no iteration
    x, info = sr.cg_restated(K, np.zeros_like(b), [(cond[0][0], 0.0)], dtype=np.float32)
    assert info["iterations"] == 0 and info["converged"] and not np.any(x)
    # a negative coefficient: breakdown at the first DOT
    Kn, _ = sr.dense_system(geom, -nu, f)
    x, info = sr.cg_restated(Kn, b, cond, dinv=np.abs(sr.dense_dinv(Kn, sr.fixed_nodes(len(b), cond))), dtype=np.float32)
    assert info["breakdown"] and not info["converged"] and info["iterations"] == 0
    # maxiter
    x, info = sr.cg_restated(K, b, cond, maxiter=3, tol=1e-6, dtype=np.float32)
    assert info["iterations"] == 3 and not info["converged"] and info["active"] and np.all(np.isfinite(x))
    # a node surrounded by nu = 0 carries no equation
    nu0 = nu.copy(); nu0[2:7, 2:7] = 0
    f0 = f.copy(); f0[2:7, 2:7] = 0
    K0, b0 = sr.dense_system(geom, nu0, f0)
    fx = sr.fixed_nodes(len(b), cond)
    dinv = sr.dense_dinv(K0, fx).reshape(9, 9)
    assert np.all(dinv[3:6, 3:6] == 0) and np.all(dinv[1:8, 1:8][nu0[1:8, 1:8] > 0] > 0)
    u = sr.dense_solve(K0, b0, cond)
    x, info = sr.cg_restated(K0, b0, cond, tol=1e-12, dtype=np.float64)
    assert info["converged"] and np.max(np.abs(x - u)) <= 1e-9 * np.max(np.abs(u)) and np.all(x.reshape(9, 9)[3:6, 3:6] == 0)


@pytest.mark.parametrize("sizes", [(9, 9), (5, 5, 5)])
def test_implicit_derivative_against_finite_differences(sizes):
    geom, nu, f, cond = small_case(sizes, 21)
    w = np.random.default_rng(8).standard_normal(geom.node_shape).ravel()
    K, b = sr.dense_system(geom, nu, f)
    u = sr.dense_solve(K, b, cond)
    lam = sr.dense_adjoint(K, w, cond)
    gnu, gf = sr.implicit_grads(geom, u, lam)
    L = lambda nu_, f_: float(w @ sr.dense_solve(*sr.dense_system(geom, nu_, f_), cond))
    rng = np.random.default_rng(9)
    for _ in range(3):
        dn, df = rng.standard_normal(geom.node_shape), rng.standard_normal(geom.node_shape)
        eps = 1e-6
        fd_nu = (L(nu + eps * dn, f) - L(nu - eps * dn, f)) / (2 * eps)
        fd_f = (L(nu, f + eps * df) - L(nu, f - eps * df)) / (2 * eps)
        assert abs(fd_nu - np.sum(gnu * dn)) <= 1e-6 * max(1.0, abs(fd_nu))
        assert abs(fd_f - np.sum(gf * df)) <= 1e-6 * max(1.0, abs(fd_f))
