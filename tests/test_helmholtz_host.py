"""CPU checks of the fused 2-D Helmholtz energy and weak-form residual (dn_helmholtz_apply, csrc/helmholtz.hip): the C ABI and its ctypes
binding agree and the library validates its arguments before any launch; the reference fixtures (tests/golden/loss_helmholtz_*.npz,
written by tools/gen_golden_helmholtz.py from the reference scripts' own `loss` bodies) agree with a float64 restatement of the operator
kept here -- the energy and `out` by the formulas of the header, not by autograd --, and that restatement agrees with central
differences and is symmetric."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_stokes_host import header_struct
from test_transport_host import GRAD_AREL, GRAD_RTOL, LOSS_RTOL

FIXTURES = ["loss_helmholtz_mms_n17.npz", "loss_helmholtz_mms_q2_n17_g3.npz", "loss_helmholtz_ddelta_n33_g3.npz",
            "loss_helmholtz_ddelta_q3_n10_g4.npz", "loss_helmholtz_mms_n17_k8.npz"]
# Tolerances of the transport fixtures (LOSS_RTOL, GRAD_RTOL, GRAD_AREL) unless the fixture's own fp32 numbers are farther than that from
# float64: then 4 x the measured distance of that fixture.  The loss distance is relative to the GROSS sum
# sum W (c nu |grad u|^2 + cr sg u^2 + |fs u f|) -- the energy is a difference --, the gradient distance to its largest entry.
# Measured (float64 restatement against the fixture):
#   mms_n17            loss 1.8e-8   gradient 2.2e-7
#   mms_q2_n17_g3      loss 2.9e-8   gradient 3.8e-7
#   ddelta_n33_g3      loss 9.4e-8   gradient 3.7e-7
#   ddelta_q3_n10_g4   loss 1.5e-7   gradient 1.9e-7
#   mms_n17_k8         loss 4.2e-8   gradient 2.0e-7
# all inside the transport figures, which therefore hold for the five.
FIXTURE_TOL = {name: (LOSS_RTOL, GRAD_RTOL, GRAD_AREL) for name in FIXTURES}


def hh_mesh(n=13, deg=2, ngp=3, B=2, ny=None):
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    gx, gw = gauss_rule(ngp)
    ny = n if ny is None else ny
    return FemGeometry(2, (n, ny), (1 / (n - 1), 1 / (ny - 1)), deg, ngp, gx, gw).mesh_struct(B)


def workspace_formula(m):
    """include/diffnet_hip.h, dn_helmholtz_args: 4160 + 16 * chunks * nely * B"""
    Q, nely = (m.nx - 1) // m.degree + 1, (m.ny - 1) // m.degree
    chunks = 1 if Q <= 64 else -(-(Q - 1) // 63)
    return 4160 + 16 * chunks * nely * m.batch


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_helmholtz_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    for s in ("dn_helmholtz_workspace_bytes", "dn_helmholtz_apply"):
        assert hasattr(h, s) and s in _lib.SYMBOLS, s
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    got = [(n, getattr(t, "_length_", 1)) for n, t in _lib.DnHelmholtzArgs._fields_]
    assert got == header_struct("dn_helmholtz_args")
    # the C layout (x86-64): 5 pointers, 3 words + 2 floats (+ padding), 2 x 40 bytes of conditions, 8 floats, 4 pointers, one int64
    assert C.sizeof(_lib.DnHelmholtzArgs) == 216 and _lib.DnHelmholtzArgs.bc.offset == 64 and _lib.DnHelmholtzArgs.out.offset == 176


def test_helmholtz_workspace_bytes_and_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    for deg, ngp, n in ((1, 2, 9), (1, 3, 9), (1, 4, 9), (2, 3, 9), (2, 4, 9), (3, 3, 10), (3, 4, 10)):
        m = hh_mesh(n, deg, ngp)
        assert h.dn_helmholtz_workspace_bytes(C.byref(m)) == workspace_formula(m), (deg, ngp)
    for n, deg, B, ny in ((257, 2, 8, None), (65, 1, 3, 9), (64, 1, 1, 64), (193, 3, 2, 10), (512, 1, 16, 512)):
        m = hh_mesh(n, deg, 3, B=B, ny=ny)
        assert h.dn_helmholtz_workspace_bytes(C.byref(m)) == workspace_formula(m), (n, deg, B)
    for field, bad in (("nsd", 3), ("nx", 1), ("ny", 0), ("batch", 0), ("ngp", 5), ("ngp", 1), ("ngp", 2), ("degree", 4), ("nx", 12)):
        m = hh_mesh()
        setattr(m, field, bad)
        assert h.dn_helmholtz_workspace_bytes(C.byref(m)) == -1, field
    m = hh_mesh()
    assert h.dn_helmholtz_apply(C.byref(m), None, None) == -1
    assert h.dn_helmholtz_apply(None, None, None) == -1
    a = _lib.DnHelmholtzArgs()                      # a NULL u
    a.out = 64
    assert h.dn_helmholtz_apply(C.byref(m), C.byref(a), None) == -1
    a.out = None
    a.u = 16                                        # a field but no output at all: rejected before anything touches the pointers
    assert h.dn_helmholtz_apply(C.byref(m), C.byref(a), None) == -1
    for name in ("energy", "sumsq"):
        setattr(a, name, 128)                       # a sum without a workspace
        assert h.dn_helmholtz_apply(C.byref(m), C.byref(a), None) == -3, name
        a.workspace, a.workspace_bytes = 256, 64    # ... or with one that is too small
        assert h.dn_helmholtz_apply(C.byref(m), C.byref(a), None) == -3, name
        a.workspace_bytes = h.dn_helmholtz_workspace_bytes(C.byref(m)) - 1
        assert h.dn_helmholtz_apply(C.byref(m), C.byref(a), None) == -3, name
        setattr(a, name, None)
        a.workspace, a.workspace_bytes = None, 0
    a.out = 64
    # a degree / ngp combination outside the domain
    for deg, ngp in ((2, 2), (3, 2), (4, 3), (0, 2), (1, 5), (1, 1)):
        mm = hh_mesh()
        mm.degree, mm.ngp, mm.nx, mm.ny = deg, ngp, 13, 13
        assert h.dn_helmholtz_apply(C.byref(mm), C.byref(a), None) == -2, (deg, ngp)
    mm = hh_mesh()
    mm.nx = 12                                      # (n - 1) % degree != 0
    assert h.dn_helmholtz_apply(C.byref(mm), C.byref(a), None) == -1
    mm = hh_mesh()
    mm.nsd = 3
    assert h.dn_helmholtz_apply(C.byref(mm), C.byref(a), None) == -1
    # BITS and BOX masks
    for k in (0, 1):
        for kind in (_lib.MASK_BITS, _lib.MASK_BOX):
            a.bc[k].mask_kind = kind
            assert h.dn_helmholtz_apply(C.byref(m), C.byref(a), None) == -2, (k, kind)
            a.bc[k].mask, a.bc[k].box_faces = 512, 15
            assert h.dn_helmholtz_apply(C.byref(m), C.byref(a), None) == -2, (k, kind)
            a.bc[k].mask, a.bc[k].box_faces = None, 0
        a.bc[k].mask_kind = 7
        assert h.dn_helmholtz_apply(C.byref(m), C.byref(a), None) == -1
        a.bc[k].mask_kind = 0
        a.bc[k].field = 120                         # a value field without its mask
        assert h.dn_helmholtz_apply(C.byref(m), C.byref(a), None) == -1
        a.bc[k].field = None
        for flag in ("mask_batched", "field_batched"):
            setattr(a.bc[k], flag, 2)
            assert h.dn_helmholtz_apply(C.byref(m), C.byref(a), None) == -1, flag
            setattr(a.bc[k], flag, 0)
    for flag in ("f_batched", "nu_batched", "sigma_batched"):
        setattr(a, flag, 2)
        assert h.dn_helmholtz_apply(C.byref(m), C.byref(a), None) == -1, flag
        setattr(a, flag, 0)
    a.f, a.f_gp = 32, 48                            # nodal and Gauss-point forcing at once
    assert h.dn_helmholtz_apply(C.byref(m), C.byref(a), None) == -1


def test_helmholtz_ops_refuse_cpu_tensors_and_bad_arguments():
    from diffnet_amd import DiffNet2DFEM, ops
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd import helmholtz as hh
    assert hh.helmholtz_coefficients(0.5) == dict(sigma=0.25, c=0.5, cr=0.5, fs=1.0)
    m = DiffNet2DFEM(None, domain_size=9, fem_basis_deg=2)
    u = torch.zeros((1, 1, 9, 9))
    with pytest.raises(DiffNetHipError):
        ops.helmholtz_apply(m.geom, u)
    for fn in (hh.helmholtz_energy_loss, hh.helmholtz_energy_loss_and_grad, hh.helmholtz_residual, hh.helmholtz_residual_loss,
               hh.helmholtz_residual_loss_and_grad):
        with pytest.raises(DiffNetHipError):
            fn(m, u, sigma=0.25)
    for fn in (hh.helmholtz_energy_loss, hh.helmholtz_energy_loss_and_grad, hh.helmholtz_residual_loss, hh.helmholtz_residual_loss_and_grad,
               hh.helmholtz_energy_loss_composed):
        with pytest.raises(ValueError):
            fn(m, u, reduction="max")
    with pytest.raises(ValueError):
        hh.helmholtz_energy_loss(m, u, bc_values=(0.0,))
    with pytest.raises(ValueError):
        ops.helmholtz_apply(m.geom, u, bc_values=(0.0,))
    with pytest.raises(ValueError):
        ops.helmholtz_apply(m.geom, u, energy_coef=(0.5, 0.5))
    with pytest.raises(ValueError):
        ops.helmholtz_apply(m.geom, u, want_out=False, want_energy=False, want_sumsq=False)


# ---------------------------------------------------------------------------------------------
# float64 restatement of the operator (include/diffnet_hip.h, dn_helmholtz_args)
# ---------------------------------------------------------------------------------------------
def helmholtz_np(u, masks, vals, hx, hy, P, ngp, nu=None, sigma=0.0, f=None, f_gp=None, ecoef=(0.5, 0.5, 1.0), ocoef=None, wscale=1.0,
                 out_scale=1.0, *, tables=None, dtype=np.float64, scale=False):
    """u: (ny, nx) float64; masks[k]: bool arrays or None; vals[k]: float or (ny, nx); nu: nodal (ny, nx) or None (1); sigma: float or
    nodal (ny, nx); f: nodal (ny, nx) or None; f_gp: (G, nely, nelx), a float or None, g = jg * ngp + ig; ecoef = (c, cr, fs); ocoef =
    (alpha, gamma, beta), None: (2c, 2cr, fs), the energy's gradient.  The formulas of the header, term by term, with the rule's
    truncated literals.  Returns dict(energy, out (ny, nx), sumsq, gross = (diffusion, reaction, forcing) sums of W c nu |grad u|^2,
    W cr |sg| u^2, W |fs u f|).  dtype: the same statements in that type, inputs, tables and constants cast once at entry; tables: see
    test_strongform_host.elem_tables; scale: the dict also holds S_energy, S_out and S_raw (S_out before out_scale), the magnitude field
    -- the same formulas with every input, table entry and constant replaced by its absolute value and every subtraction made an
    addition, after the Dirichlet substitutions; 0 on the Dirichlet nodes -- and `raw`, out before out_scale."""
    from test_strongform_host import elem_tables
    dt = np.dtype(dtype).type
    ny, nx = np.shape(u)
    nely, nelx = (ny - 1) // P, (nx - 1) // P
    nb = P + 1
    fixed = np.zeros((ny, nx), dtype=bool)
    for k in (0, 1):
        if masks[k] is not None:
            fixed |= np.asarray(masks[k], dtype=bool)

    def loc(jb, ib):
        return (slice(jb, jb + P * (nely - 1) + 1, P), slice(ib, ib + P * (nelx - 1) + 1, P))

    def run(A, minus):
        c = lambda x: A(np.asarray(x, dtype=dt))                                # noqa: E731
        Bt, Dt, _, Wt = (c(t) for t in elem_tables(P, ngp, tables, dt, wscale))
        cc, cr, fs = (c(x)[()] for x in ecoef)
        alpha, gamma, beta = (dt(2) * cc, dt(2) * cr, fs) if ocoef is None else (c(x)[()] for x in ocoef)
        sx, sy = dt(2) / dt(hx), dt(2) / dt(hy)
        ut = c(u)
        for k in (0, 1):                            # in order: where both hold, condition 2's value is the one used
            if masks[k] is not None:
                ut = np.where(masks[k], c(vals[k]), ut)
        energy, out = dt(0), np.zeros((ny, nx), dtype=dt)
        gross = [dt(0), dt(0), dt(0)]
        for jg in range(ngp):
            for ig in range(ngp):
                g, W = jg * ngp + ig, Wt[jg, ig]
                N = {(jb, ib): Bt[ig, ib] * Bt[jg, jb] for jb in range(nb) for ib in range(nb)}
                Nx = {(jb, ib): Dt[ig, ib] * sx * Bt[jg, jb] for jb in range(nb) for ib in range(nb)}
                Ny = {(jb, ib): Bt[ig, ib] * Dt[jg, jb] * sy for jb in range(nb) for ib in range(nb)}

                def at(t, tab):
                    return sum(tab[a] * t[loc(*a)] for a in tab)

                v, ux, uy = at(ut, N), at(ut, Nx), at(ut, Ny)
                nug = np.ones((nely, nelx), dtype=dt) if nu is None else at(c(nu), N)
                sgg = np.full((nely, nelx), c(float(sigma)), dtype=dt) if np.ndim(sigma) == 0 else at(c(sigma), N)
                if f is not None:
                    fg = at(c(f), N)
                elif f_gp is None or np.ndim(f_gp) == 0:
                    fg = np.full((nely, nelx), c(0.0 if f_gp is None else float(f_gp)), dtype=dt)
                else:
                    fg = c(f_gp)[g]
                diff, react, forc = cc * nug * (ux * ux + uy * uy), cr * sgg * v * v, fs * v * fg
                energy += W * np.sum(diff + minus * react + minus * forc)
                gross[0] += W * np.sum(np.abs(diff))
                gross[1] += W * np.sum(np.abs(react))
                gross[2] += W * np.sum(np.abs(forc))
                for a in N:
                    out[loc(*a)] += W * (alpha * nug * (Nx[a] * ux + Ny[a] * uy) + minus * gamma * sgg * N[a] * v + minus * beta * N[a] * fg)
        out = np.where(fixed, dt(0), out)
        assert out.dtype == dt, out.dtype                                          # numpy promotes silently
        return dict(energy=energy, out=out * c(out_scale), raw=out, sumsq=float(np.sum(out * out)), gross=tuple(gross))

    res = run(lambda x: x, dt(-1))
    if scale:
        mag = run(np.abs, dt(1))
        res.update(S_energy=mag["energy"], S_out=mag["out"], S_raw=mag["raw"])
    return res


def fixture_case(z):
    kw = eval(str(z["kwargs"]))
    n, P = kw["domain_size"], kw.get("fem_basis_deg", 1)
    nel = (n - 1) // P
    h = 1.0 / nel
    return dict(masks=[z["mask1"][0, 0] != 0, z["mask2"][0, 0] != 0], vals=[1.0, 0.0], hx=h, hy=h, P=P, ngp=kw.get("ngp_1d", 2),
                nu=z["inputs"][0, 0].astype(np.float64), sigma=float(z["khh"]) ** 2, f=z["forcing"][0, 0].astype(np.float64),
                out_scale=1.0 / (nel * nel))


def fixture_distances(name):
    z = np.load(os.path.join(GOLDEN, name))
    c = fixture_case(z)
    r = helmholtz_np(z["u"][0, 0].astype(np.float64), **c)
    loss, gross = r["energy"] * c["out_scale"], sum(r["gross"]) * c["out_scale"]
    ref = z["grad"][0, 0]
    return z, c, r, abs(loss - float(z["loss"])) / gross, np.abs(r["out"] - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("name", FIXTURES)
def test_helmholtz_fixtures_agree_with_float64_restatement(name):
    z, c, r, dl, dg = fixture_distances(name)
    print(name, "loss / gross", dl, "grad", dg)
    lrt, grt, gar = FIXTURE_TOL[name]
    ref = z["grad"][0, 0]
    assert dl <= lrt, (name, dl)
    np.testing.assert_allclose(r["out"], ref, rtol=grt, atol=gar * np.abs(ref).max())
    assert np.all(ref[c["masks"][0] | c["masks"][1]] == 0.0)            # the reference's torch.where passes no gradient to a Dirichlet node


def test_helmholtz_fixtures_hold_what_they_should():
    shares = {}
    for name in FIXTURES:
        z, c, r, _, _ = fixture_distances(name)
        for k in ("kwargs", "u", "inputs", "forcing", "mask1", "mask2", "khh", "loss", "grad"):
            assert k in z.files, (name, k)
        assert z["mask2"].any(), name               # the datasets leave condition 1 empty: the central-difference and GPU tests cover it
        assert z["u"].shape[0] == 1 and np.abs(z["u"]).max() < 0.6            # the smooth field, not order-one noise
        d, s, f = r["gross"]
        shares[name] = (d / (d + s + f), s / (d + s + f))
        print(name, "diffusion share", shares[name][0], "reaction share", shares[name][1])
        assert shares[name][1] >= 20 * FIXTURE_TOL[name][0], (name, shares[name])
    assert float(np.load(os.path.join(GOLDEN, FIXTURES[4]))["khh"]) == 8.0
    assert shares[FIXTURES[4]][1] > shares[FIXTURES[4]][0]                    # k^2 = 64 > 2 pi^2: the reaction term outweighs the diffusion


# ---------------------------------------------------------------------------------------------
# the restatement against central differences; symmetry
# ---------------------------------------------------------------------------------------------
def cd_case(P, ngp, nx, ny, seed=11):
    rs = np.random.default_rng(seed + P)
    m1, m2 = rs.random((ny, nx)) < 0.2, rs.random((ny, nx)) < 0.2
    m1[0, 0] = m2[0, 0] = True                      # the two conditions overlap
    m1[1, 1], m2[1, 1] = False, False
    u = 2 * rs.random((ny, nx)) - 1
    c = dict(masks=[m1, m2], vals=[2 * rs.random((ny, nx)) - 1, 2 * rs.random((ny, nx)) - 1], hx=0.2, hy=0.25, P=P, ngp=ngp,
             nu=0.5 + rs.random((ny, nx)), sigma=4.0 * rs.random((ny, nx)) - 1.0, f=rs.random((ny, nx)) - 0.5, ecoef=(0.7, 0.4, 0.9),
             wscale=0.8, out_scale=0.37)
    return u, c


@pytest.mark.parametrize("P,ngp,nx,ny", [(1, 2, 6, 5), (2, 3, 7, 5), (3, 4, 7, 4)])
def test_helmholtz_gradient_of_the_restatement_equals_central_differences(P, ngp, nx, ny):
    u, c = cd_case(P, ngp, nx, ny)
    m1, m2 = c["masks"]
    grad = helmholtz_np(u, **c)["out"]
    assert np.abs(grad).max() > 1e-2 and np.all(grad[m1 | m2] == 0.0)
    eps = 1e-6
    fd = np.zeros_like(u)
    for j in range(ny):
        for i in range(nx):
            up, um = u.copy(), u.copy()
            up[j, i] += eps
            um[j, i] -= eps
            fd[j, i] = c["out_scale"] * (helmholtz_np(up, **c)["energy"] - helmholtz_np(um, **c)["energy"]) / (2 * eps)
    np.testing.assert_allclose(grad, fd, rtol=0, atol=1e-8 * np.abs(fd).max())
    # out for alpha = gamma = beta = 1 is the gradient of the energy with c = cr = 0.5, fs = 1
    r1 = helmholtz_np(u, **dict(c, ecoef=(0.0, 0.0, 0.0), ocoef=(1.0, 1.0, 1.0)))
    r2 = helmholtz_np(u, **dict(c, ecoef=(0.5, 0.5, 1.0), ocoef=None))
    np.testing.assert_allclose(r1["out"], r2["out"], rtol=0, atol=1e-14 * np.abs(r2["out"]).max())
    np.testing.assert_allclose(r1["sumsq"], np.sum((r1["out"] / c["out_scale"]) ** 2), rtol=1e-13)
    # with Gauss-point forcing and a constant sigma, one node
    c2 = dict(c, f=None, f_gp=np.random.default_rng(3).random((ngp * ngp, (ny - 1) // P, (nx - 1) // P)), sigma=3.0, nu=None)
    grad2 = helmholtz_np(u, **c2)["out"]
    up, um = u.copy(), u.copy()
    up[1, 1] += eps
    um[1, 1] -= eps
    fd2 = c["out_scale"] * (helmholtz_np(up, **c2)["energy"] - helmholtz_np(um, **c2)["energy"]) / (2 * eps)
    np.testing.assert_allclose(grad2[1, 1], fd2, rtol=0, atol=1e-8 * np.abs(grad2).max())


@pytest.mark.parametrize("P,ngp,nx,ny", [(1, 2, 6, 5), (2, 3, 7, 5), (3, 4, 7, 4)])
def test_helmholtz_restatement_operator_is_symmetric(P, ngp, nx, ny):
    """<v, A w> = <w, A v> for the homogeneous operator (no forcing, zero Dirichlet values): what the residual loss's backward uses"""
    _, c = cd_case(P, ngp, nx, ny)
    rs = np.random.default_rng(77)
    c = dict(c, vals=[0.0, 0.0], f=None, ecoef=(0.0, 0.0, 0.0), ocoef=(1.0, 1.0, 0.0), out_scale=1.0)
    v, w = 2 * rs.random((ny, nx)) - 1, 2 * rs.random((ny, nx)) - 1
    free = ~(c["masks"][0] | c["masks"][1])
    Av, Aw = helmholtz_np(v, **c)["out"], helmholtz_np(w, **c)["out"]
    a, b = np.sum((v * free) * Aw), np.sum((w * free) * Av)
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)) and abs(a) > 1e-3
