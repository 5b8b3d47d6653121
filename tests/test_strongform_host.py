"""CPU checks of the fused 2-D strong-form least-squares loss (dn_strongform_apply, csrc/strongform.hip): the C ABI and its ctypes binding
agree and the library validates its arguments before any launch; the reference fixtures (tests/golden/loss_strongform_*.npz, written by
tools/gen_golden_strongform.py from the reference scripts' own `loss` bodies) agree with a float64 restatement of the operator kept
here -- the sum and the gradient by the formula of the header, not by autograd --, and that gradient agrees with central differences."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_stokes_host import header_struct
from test_transport_host import GRAD_AREL, GRAD_RTOL, LOSS_RTOL

FIXTURES = ["loss_strongform_burgers_n17.npz", "loss_strongform_poisson_q3_n10.npz", "loss_strongform_poisson_q3_n10_g4.npz"]
# Tolerances of the transport fixtures (LOSS_RTOL, GRAD_RTOL, GRAD_AREL) unless the fixture's own fp32 numbers are farther than that from
# float64 (the reference sums (2/h)^2-sized second derivatives in fp32): then 4 x the measured distance of that fixture.
# Measured (float64 restatement against the fixture; loss relative, gradient relative to its largest entry):
#   burgers_n17        loss 5.4e-8   gradient 1.9e-7
#   poisson_q3_n10     loss 4.7e-8   gradient 1.1e-7
#   poisson_q3_n10_g4  loss 5.0e-8   gradient 7.0e-8
# all inside the transport figures, which therefore hold for the three.
FIXTURE_TOL = {name: (LOSS_RTOL, GRAD_RTOL, GRAD_AREL) for name in FIXTURES}


def sf_mesh(n=13, deg=2, ngp=3, B=2, ny=None):
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    gx, gw = gauss_rule(ngp)
    ny = n if ny is None else ny
    return FemGeometry(2, (n, ny), (1 / (n - 1), 1 / (ny - 1)), deg, ngp, gx, gw).mesh_struct(B)


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_strongform_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    for s in ("dn_strongform_workspace_bytes", "dn_strongform_apply"):
        assert hasattr(h, s) and s in _lib.SYMBOLS, s
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    got = [(n, getattr(t, "_length_", 1)) for n, t in _lib.DnStrongformArgs._fields_]
    assert got == header_struct("dn_strongform_args")
    assert [(n, getattr(t, "_length_", 1)) for n, t in _lib.DnDirichlet._fields_] == header_struct("dn_dirichlet")
    # the C layout (x86-64): 3 pointers, 2 words, 2 x 40 bytes of conditions, 8 floats, 16 floats, 4 pointers, one int64
    assert C.sizeof(_lib.DnStrongformArgs) == 248 and _lib.DnStrongformArgs.d2basis.offset == 144 and _lib.DnStrongformArgs.grad.offset == 216


def test_strongform_workspace_bytes_and_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    for deg, ngp, n in ((1, 2, 9), (1, 3, 9), (1, 4, 9), (2, 3, 9), (2, 4, 9), (3, 3, 10), (3, 4, 10)):
        assert h.dn_strongform_workspace_bytes(C.byref(sf_mesh(n, deg, ngp))) > 64 * 65, (deg, ngp)
    big = h.dn_strongform_workspace_bytes(C.byref(sf_mesh(257, 2, 3, B=8)))
    assert big > 64 * 65 and (big - 64 * 65) % 8 == 0              # the header + doubles
    for field, bad in (("nsd", 3), ("nx", 1), ("ny", 0), ("batch", 0), ("ngp", 5), ("ngp", 1), ("ngp", 2), ("degree", 4), ("nx", 12)):
        m = sf_mesh()
        setattr(m, field, bad)
        assert h.dn_strongform_workspace_bytes(C.byref(m)) == -1, field
    m = sf_mesh()
    assert h.dn_strongform_apply(C.byref(m), None, None) == -1
    assert h.dn_strongform_apply(None, None, None) == -1
    a = _lib.DnStrongformArgs()                     # a NULL u
    a.grad = 64
    assert h.dn_strongform_apply(C.byref(m), C.byref(a), None) == -1
    a.grad = None
    a.u = 16                                        # a field but no output at all: rejected before anything touches the pointers
    assert h.dn_strongform_apply(C.byref(m), C.byref(a), None) == -1
    a.sum = 128                                     # sum without a workspace
    assert h.dn_strongform_apply(C.byref(m), C.byref(a), None) == -3
    a.workspace, a.workspace_bytes = 256, 64        # ... or with one that is too small
    assert h.dn_strongform_apply(C.byref(m), C.byref(a), None) == -3
    a.workspace_bytes = h.dn_strongform_workspace_bytes(C.byref(m)) - 1
    assert h.dn_strongform_apply(C.byref(m), C.byref(a), None) == -3
    a.sum, a.workspace, a.workspace_bytes = None, None, 0
    a.grad = 64
    # a degree / ngp combination outside the rule
    for deg, ngp in ((2, 2), (3, 2), (4, 3), (0, 2), (1, 5), (1, 1)):
        mm = sf_mesh()
        mm.degree, mm.ngp, mm.nx, mm.ny = deg, ngp, 13, 13
        assert h.dn_strongform_apply(C.byref(mm), C.byref(a), None) == -2, (deg, ngp)
    mm = sf_mesh()
    mm.nx = 12                                      # (n - 1) % degree != 0
    assert h.dn_strongform_apply(C.byref(mm), C.byref(a), None) == -1
    mm = sf_mesh()
    mm.nsd = 3
    assert h.dn_strongform_apply(C.byref(mm), C.byref(a), None) == -1
    # BITS and BOX masks
    for k in (0, 1):
        for kind in (_lib.MASK_BITS, _lib.MASK_BOX):
            a.bc[k].mask_kind = kind
            assert h.dn_strongform_apply(C.byref(m), C.byref(a), None) == -2, (k, kind)
            a.bc[k].mask, a.bc[k].box_faces = 512, 15
            assert h.dn_strongform_apply(C.byref(m), C.byref(a), None) == -2, (k, kind)
            a.bc[k].mask, a.bc[k].box_faces = None, 0
        a.bc[k].mask_kind = 7
        assert h.dn_strongform_apply(C.byref(m), C.byref(a), None) == -1
        a.bc[k].mask_kind = 0
        a.bc[k].field = 120                         # a value field without its mask
        assert h.dn_strongform_apply(C.byref(m), C.byref(a), None) == -1
        a.bc[k].field = None
        for flag in ("mask_batched", "field_batched"):
            setattr(a.bc[k], flag, 2)
            assert h.dn_strongform_apply(C.byref(m), C.byref(a), None) == -1, flag
            setattr(a.bc[k], flag, 0)
    a.f_batched = 2
    assert h.dn_strongform_apply(C.byref(m), C.byref(a), None) == -1
    a.f_batched = 0
    a.f, a.f_gp = 32, 48                            # nodal and Gauss-point forcing at once
    assert h.dn_strongform_apply(C.byref(m), C.byref(a), None) == -1


def test_strongform_ops_refuse_cpu_tensors_and_bad_arguments():
    from diffnet_amd import DiffNet2DFEM, ops
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd.strongform import burgers_coefficients, poisson_strong_coefficients, strong_form_loss, strong_form_loss_and_grad
    assert burgers_coefficients() == (0.0, 1.0, 1.0, 0.0, 0.0, 0.0)
    assert burgers_coefficients(0.01 / np.pi) == (0.0, 1.0, 1.0, -0.01 / np.pi, 0.0, 0.0)
    assert poisson_strong_coefficients() == (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    m = DiffNet2DFEM(None, domain_size=9, fem_basis_deg=2)
    u = torch.zeros((1, 1, 9, 9))
    with pytest.raises(DiffNetHipError):
        ops.strongform_apply(m.geom, u, coef=burgers_coefficients())
    with pytest.raises(DiffNetHipError):
        strong_form_loss(m, u, coef=burgers_coefficients())
    with pytest.raises(DiffNetHipError):
        strong_form_loss_and_grad(m, u, coef=burgers_coefficients())
    with pytest.raises(ValueError):
        strong_form_loss(m, u, coef=burgers_coefficients(), reduction="max")
    with pytest.raises(ValueError):
        strong_form_loss(m, u, coef=(1.0, 0.0))
    with pytest.raises(ValueError):
        ops.strongform_apply(m.geom, u, bc_values=(0.0,))
    with pytest.raises(ValueError):
        ops.strongform_apply(m.geom, u, want_grad=False, want_sum=False)


# ---------------------------------------------------------------------------------------------
# float64 restatement of the operator (include/diffnet_hip.h, dn_strongform_args)
# ---------------------------------------------------------------------------------------------
def elem_tables(P, ngp, tables, dt, wscale):
    """The 1-D tables (N, dN, d2N, each (ngp, P + 1)) and the 2-D weights W[jg][ig] of a restatement in the type dt.  tables None: the
    rule's own, W = wscale w_ig w_jg; else the (N, dN, d2N, w) given -- the float32 values of the mesh struct -- with the weights formed
    as the host forms them, w_jg * (w_ig * wscale) in float32 (elem2d_fill, csrc/elem2d_common.h)."""
    from diffnet_amd.tables import Basis1D, gauss_rule
    if tables is None:
        gx, gw = gauss_rule(ngp)
        Bt, Dt, D2t = Basis1D(P).at_gauss(gx)       # (ngp, nbf)
        gw = np.asarray(gw, dtype=dt)
        W = [[dt(wscale) * gw[ig] * gw[jg] for ig in range(ngp)] for jg in range(ngp)]
    else:
        Bt, Dt, D2t, gw = tables
        w32 = np.asarray(gw, dtype=np.float32)
        W = [[dt(w32[jg] * (w32[ig] * np.float32(wscale))) for ig in range(ngp)] for jg in range(ngp)]
    return np.asarray(Bt, dtype=dt), np.asarray(Dt, dtype=dt), np.asarray(D2t, dtype=dt), np.asarray(W, dtype=dt)


def strongform_np(u, masks, vals, coef, hx, hy, P, ngp, f=None, f_gp=None, wscale=1.0, out_scale=1.0, *, tables=None, dtype=np.float64,
                  scale=False):
    """u: (ny, nx) float64; masks[k]: bool arrays or None; vals[k]: float or (ny, nx); f: nodal (ny, nx) or None; f_gp: (G, nely, nelx), a
    float or None, g = jg * ngp + ig.  The formulas of the header, term by term, with the rule's truncated literals.
    Returns (sum, grad (ny, nx), r (G, nely, nelx)).  dtype: the same statements in that type, inputs, tables and constants cast once at
    entry; tables: see elem_tables; scale: also returns (S_sum, S_grad), the magnitude field -- the same formulas with every input,
    table entry and constant replaced by its absolute value (there is no subtraction), after the Dirichlet substitutions; S_grad is 0 on
    the Dirichlet nodes."""
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

    def run(A):
        c = lambda x: A(np.asarray(x, dtype=dt))                                # noqa: E731
        Bt, Dt, D2t, Wt = (c(t) for t in elem_tables(P, ngp, tables, dt, wscale))
        ax, ay, b, dxx, dyy, fs = (c(x)[()] for x in coef)
        sx, sy = dt(2) / dt(hx), dt(2) / dt(hy)
        ut = c(u)
        for k in (0, 1):                            # in order: where both hold, condition 2's value is the one used
            if masks[k] is not None:
                ut = np.where(masks[k], c(vals[k]), ut)
        total, grad = dt(0), np.zeros((ny, nx), dtype=dt)
        r_all = np.zeros((ngp * ngp, nely, nelx), dtype=dt)
        for jg in range(ngp):
            for ig in range(ngp):
                g, W = jg * ngp + ig, Wt[jg, ig]
                N = {(jb, ib): Bt[ig, ib] * Bt[jg, jb] for jb in range(nb) for ib in range(nb)}
                Nx = {(jb, ib): Dt[ig, ib] * sx * Bt[jg, jb] for jb in range(nb) for ib in range(nb)}
                Ny = {(jb, ib): Bt[ig, ib] * Dt[jg, jb] * sy for jb in range(nb) for ib in range(nb)}
                Nxx = {(jb, ib): D2t[ig, ib] * sx * sx * Bt[jg, jb] for jb in range(nb) for ib in range(nb)}
                Nyy = {(jb, ib): Bt[ig, ib] * D2t[jg, jb] * sy * sy for jb in range(nb) for ib in range(nb)}

                def at(t, tab):
                    return sum(tab[a] * t[loc(*a)] for a in tab)

                v, ux, uy, uxx, uyy = at(ut, N), at(ut, Nx), at(ut, Ny), at(ut, Nxx), at(ut, Nyy)
                if f is not None:
                    fg = at(c(f), N)
                elif f_gp is None or np.ndim(f_gp) == 0:
                    fg = np.full((nely, nelx), c(0.0 if f_gp is None else float(f_gp)), dtype=dt)
                else:
                    fg = c(f_gp)[g]
                r = ax * ux + ay * uy + b * v * ux + dxx * uxx + dyy * uyy + fs * fg
                r_all[g] = r
                total += W * np.sum(r * r)
                for a in N:
                    grad[loc(*a)] += dt(2) * W * r * (ax * Nx[a] + ay * Ny[a] + b * (N[a] * ux + v * Nx[a]) + dxx * Nxx[a] + dyy * Nyy[a])
        grad = np.where(fixed, dt(0), grad) * c(out_scale)
        assert grad.dtype == dt and r_all.dtype == dt, (grad.dtype, r_all.dtype)       # numpy promotes silently
        return total, grad, r_all

    total, grad, r_all = run(lambda x: x)
    if not scale:
        return total, grad, r_all
    S_total, S_grad, _ = run(np.abs)
    return total, grad, r_all, (S_total, S_grad)


def fixture_case(z):
    kw = eval(str(z["kwargs"]))
    n, P = kw["domain_size"], kw["fem_basis_deg"]
    nel = (n - 1) // P
    h = 1.0 / nel
    v1 = z["v1"].astype(np.float64)
    return dict(masks=[z["mask1"][0, 0] != 0, z["mask2"][0, 0] != 0], vals=[v1 if v1.ndim else float(v1), 0.0], coef=tuple(z["coef"]),
                hx=h, hy=h, P=P, ngp=kw.get("ngp_1d", 3), f=z["forcing"][0, 0].astype(np.float64), wscale=float(z["wscale"]),
                out_scale=1.0 / (nel * nel))


@pytest.mark.parametrize("name", FIXTURES)
def test_strongform_fixtures_agree_with_float64_restatement(name):
    z = np.load(os.path.join(GOLDEN, name))
    c = fixture_case(z)
    total, grad, _ = strongform_np(z["u"][0, 0].astype(np.float64), **c)
    loss = total * c["out_scale"]
    ref = z["grad"][0, 0]
    print(name, "loss rel", abs(loss - float(z["loss"])) / float(z["loss"]), "grad", np.abs(grad - ref).max() / np.abs(ref).max())
    lrt, grt, gar = FIXTURE_TOL[name]
    np.testing.assert_allclose(loss, float(z["loss"]), rtol=lrt)
    np.testing.assert_allclose(grad, ref, rtol=grt, atol=gar * np.abs(ref).max())
    assert np.all(ref[c["masks"][0] | c["masks"][1]] == 0.0)            # the reference's torch.where passes no gradient to a Dirichlet node


def test_strongform_fixtures_hold_what_they_should():
    for name in FIXTURES:
        z = np.load(os.path.join(GOLDEN, name))
        for k in ("kwargs", "u", "inputs", "forcing", "coef", "loss", "grad", "mask1", "mask2", "v1"):
            assert k in z.files, (name, k)
        assert np.abs(z["u"]).max() <= 1.0 and np.abs(z["u"]).std() > 0.2         # order-one random, not a smooth solution
    z = np.load(os.path.join(GOLDEN, FIXTURES[0]))
    assert tuple(z["coef"]) == (0.0, 1.0, 1.0, 0.0, 0.0, 0.0) and (z["mask1"] & z["mask2"]).any() and z["v1"].ndim == 2
    z = np.load(os.path.join(GOLDEN, FIXTURES[1]))
    assert tuple(z["coef"]) == (0.0, 0.0, 0.0, 1.0, 1.0, 1.0) and np.abs(z["forcing"]).max() > 1.0


@pytest.mark.parametrize("P,ngp,nx,ny", [(2, 3, 7, 5), (3, 4, 7, 4), (1, 2, 5, 4)])
def test_strongform_gradient_of_the_restatement_equals_central_differences(P, ngp, nx, ny):
    """float64 central differences of the sum; the Q2 case is the 7 x 5-node mesh with b != 0 and dxx != 0"""
    rs = np.random.default_rng(5 + P)
    u = 2 * rs.random((ny, nx)) - 1
    m1, m2 = rs.random((ny, nx)) < 0.2, rs.random((ny, nx)) < 0.2
    m1[0, 0] = m2[0, 0] = True
    c = dict(masks=[m1, m2], vals=[2 * rs.random((ny, nx)) - 1, 0.3], coef=(0.7, -0.4, 1.3, -0.05, 0.02, 0.9), hx=0.2, hy=0.25, P=P, ngp=ngp,
             f=rs.random((ny, nx)) - 0.5, wscale=0.8, out_scale=0.37)
    _, grad, _ = strongform_np(u, **c)
    assert np.abs(grad).max() > 1e-2 and np.all(grad[m1 | m2] == 0.0)
    eps = 1e-6
    fd = np.zeros_like(u)
    for j in range(ny):
        for i in range(nx):
            up, um = u.copy(), u.copy()
            up[j, i] += eps
            um[j, i] -= eps
            fd[j, i] = c["out_scale"] * (strongform_np(up, **c)[0] - strongform_np(um, **c)[0]) / (2 * eps)
    np.testing.assert_allclose(grad, fd, rtol=0, atol=1e-7 * np.abs(fd).max())
    # without the nonlinear and the second-order terms, and with Gauss-point forcing
    c2 = dict(c, coef=(0.7, -0.4, 0.0, 0.0, 0.0, 0.9), f=None, f_gp=rs.random((ngp * ngp, (ny - 1) // P, (nx - 1) // P)))
    _, grad2, _ = strongform_np(u, **c2)
    j, i = np.argwhere(~(m1 | m2))[0]
    up, um = u.copy(), u.copy()
    up[j, i] += eps
    um[j, i] -= eps
    fd2 = c["out_scale"] * (strongform_np(up, **c2)[0] - strongform_np(um, **c2)[0]) / (2 * eps)
    np.testing.assert_allclose(grad2[j, i], fd2, rtol=0, atol=1e-7 * np.abs(grad2).max())
