"""CPU checks of the fused 2-D first-order-system least-squares loss (dn_fosls_apply, csrc/fosls.hip): the C ABI and its ctypes binding
agree and the library validates its arguments before any launch; the reference fixtures (tests/golden/loss_fosls_*.npz, written by
tools/gen_golden_fosls.py from the reference script's own `loss` body) agree with a float64 restatement of the operator kept here -- the
sum and the three gradients by the formulas of the header, not by autograd --, and those gradients agree with central differences."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_stokes_host import header_struct
from test_transport_host import GRAD_AREL, GRAD_RTOL, LOSS_RTOL

FIXTURES = ["loss_fosls_q1_n9.npz", "loss_fosls_q1_n9_g3.npz", "loss_fosls_q2_n9.npz", "loss_fosls_q3_n10_g4.npz"]
# Tolerances of the transport fixtures (LOSS_RTOL, GRAD_RTOL, GRAD_AREL = 1e-5, 1e-4, 1e-4) unless the fixture's own fp32 numbers are
# farther than that from float64: then 4 x the measured distance of that fixture.
# Measured (float64 restatement against the fixture; loss relative, gradient relative to its largest entry):
#   q1_n9      loss 1.2e-9   gradient 1.1e-7
#   q1_n9_g3   loss 5.1e-8   gradient 2.1e-7
#   q2_n9      loss 4.9e-8   gradient 1.5e-7
#   q3_n10_g4  loss 3.8e-8   gradient 1.7e-7
# all inside the transport figures (first derivatives only), which therefore hold for the four.
FIXTURE_TOL = {name: (LOSS_RTOL, GRAD_RTOL, GRAD_AREL) for name in FIXTURES}


def fo_mesh(n=13, deg=2, ngp=3, B=2, ny=None):
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    gx, gw = gauss_rule(ngp)
    ny = n if ny is None else ny
    return FemGeometry(2, (n, ny), (1 / (n - 1), 1 / (ny - 1)), deg, ngp, gx, gw).mesh_struct(B)


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_fosls_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    for s in ("dn_fosls_workspace_bytes", "dn_fosls_apply"):
        assert hasattr(h, s) and s in _lib.SYMBOLS, s
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    got = [(n, getattr(t, "_length_", 1)) for n, t in _lib.DnFoslsArgs._fields_]
    assert got == header_struct("dn_fosls_args")
    assert [(n, getattr(t, "_length_", 1)) for n, t in _lib.DnDirichlet._fields_] == header_struct("dn_dirichlet")
    # the C layout (x86-64): 3 pointers + int64, pointer + 2 words, 2 pointers + 2 words, 2 x 40 bytes of conditions, 5 floats (+ 4 bytes
    # of padding), 4 pointers, int64, 2 pointers, int64
    A = _lib.DnFoslsArgs
    assert C.sizeof(A) == 240 and A.field_stride.offset == 24 and A.bc.offset == 72 and A.wq.offset == 152 and A.in_scale.offset == 176
    assert A.grad_stride.offset == 208 and A.workspace_bytes.offset == 232


def _valid_args(_lib, m):
    a = _lib.DnFoslsArgs()
    a.u, a.mx, a.my = 16, 32, 48
    a.field_stride = a.grad_stride = m.nx * m.ny
    a.grad_u = 64
    return a


def test_fosls_workspace_bytes_and_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    for deg, ngp, n in ((1, 2, 9), (1, 3, 9), (1, 4, 9), (2, 3, 9), (2, 4, 9), (3, 3, 10), (3, 4, 10)):
        assert h.dn_fosls_workspace_bytes(C.byref(fo_mesh(n, deg, ngp))) == 64 * 65 + 8 * ((n - 1) // deg) * 2, (deg, ngp)
    # one partial sum per (one-wave chunk, element row, sample): 257 nodes of Q2 = 129 thread columns = 3 chunks of 63 + 1
    assert h.dn_fosls_workspace_bytes(C.byref(fo_mesh(257, 2, 3, B=8))) == 64 * 65 + 8 * 3 * 128 * 8
    assert h.dn_fosls_workspace_bytes(C.byref(fo_mesh(512, 1, 2, B=1))) == 64 * 65 + 8 * 9 * 511
    for field, bad in (("nsd", 3), ("nx", 1), ("ny", 0), ("batch", 0), ("ngp", 5), ("ngp", 1), ("ngp", 2), ("degree", 4), ("nx", 12)):
        m = fo_mesh()
        setattr(m, field, bad)
        assert h.dn_fosls_workspace_bytes(C.byref(m)) == -1, field
    m = fo_mesh()
    assert h.dn_fosls_apply(C.byref(m), None, None) == -1
    assert h.dn_fosls_apply(None, None, None) == -1
    for missing in ("u", "mx", "my"):               # a NULL field
        a = _valid_args(_lib, m)
        setattr(a, missing, None)
        assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -1, missing
    a = _valid_args(_lib, m)
    a.grad_u = None                                 # fields but no output at all: rejected before anything touches the pointers
    assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -1
    a.sum = 128                                     # sum without a workspace
    assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -3
    a.workspace, a.workspace_bytes = 256, 64        # ... or with one that is too small
    assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -3
    a.workspace_bytes = h.dn_fosls_workspace_bytes(C.byref(m)) - 1
    assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -3
    # a batch stride smaller than one node image
    for which in ("field_stride", "grad_stride"):
        for gname in ("grad_u", "grad_mx", "grad_my"):
            a = _valid_args(_lib, m)
            a.grad_u = None
            setattr(a, gname, 64)
            setattr(a, which, m.nx * m.ny - 1)
            assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -1, (which, gname)
            setattr(a, which, 0)
            assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -1, (which, gname)
    a = _valid_args(_lib, m)
    # a degree / ngp combination outside the rule
    for deg, ngp in ((2, 2), (3, 2), (4, 3), (0, 2), (1, 5), (1, 1)):
        mm = fo_mesh()
        mm.degree, mm.ngp, mm.nx, mm.ny = deg, ngp, 13, 13
        assert h.dn_fosls_apply(C.byref(mm), C.byref(a), None) == -2, (deg, ngp)
    mm = fo_mesh()
    mm.nx = 12                                      # (n - 1) % degree != 0
    assert h.dn_fosls_apply(C.byref(mm), C.byref(a), None) == -1
    mm = fo_mesh()
    mm.nsd = 3
    assert h.dn_fosls_apply(C.byref(mm), C.byref(a), None) == -1
    # BITS and BOX masks
    for k in (0, 1):
        for kind in (_lib.MASK_BITS, _lib.MASK_BOX):
            a.bc[k].mask_kind = kind
            assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -2, (k, kind)
            a.bc[k].mask, a.bc[k].box_faces = 512, 15
            assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -2, (k, kind)
            a.bc[k].mask, a.bc[k].box_faces = None, 0
        a.bc[k].mask_kind = 7
        assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -1
        a.bc[k].mask_kind = 0
        a.bc[k].field = 120                         # a value field without its mask
        assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -1
        a.bc[k].field = None
        for flag in ("mask_batched", "field_batched"):
            setattr(a.bc[k], flag, 2)
            assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -1, flag
            setattr(a.bc[k], flag, 0)
    for flag in ("f_batched", "nu_batched"):
        setattr(a, flag, 2)
        assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -1, flag
        setattr(a, flag, 0)
    a.f, a.f_gp = 32, 48                            # nodal and Gauss-point forcing at once
    assert h.dn_fosls_apply(C.byref(m), C.byref(a), None) == -1


def test_fosls_ops_refuse_cpu_tensors_and_bad_arguments():
    from diffnet_amd import DiffNet2DFEM, ops
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd.fosls import fosls_loss, fosls_loss_and_grad
    m = DiffNet2DFEM(None, domain_size=9, fem_basis_deg=1)
    u, mx, my = (torch.zeros((1, 1, 9, 9)) for _ in range(3))
    packed = torch.zeros((1, 3, 9, 9))
    with pytest.raises(DiffNetHipError):
        ops.fosls_apply(m.geom, u, mx, my)
    with pytest.raises(DiffNetHipError):
        ops.fosls_apply(m.geom, fields=packed)
    with pytest.raises(DiffNetHipError):
        fosls_loss(m, u, mx, my)
    with pytest.raises(DiffNetHipError):
        fosls_loss(m, packed)
    with pytest.raises(DiffNetHipError):
        fosls_loss_and_grad(m, packed)
    with pytest.raises(ValueError):
        fosls_loss(m, u, mx, my, reduction="max")
    with pytest.raises(ValueError):
        fosls_loss(m, u, mx, my, weights=(1.0,))
    with pytest.raises(ValueError):
        fosls_loss(m, u, mx)                                        # two of the three fields
    with pytest.raises(ValueError):
        fosls_loss(m, torch.zeros((1, 2, 9, 9)))                    # a packed tensor with the wrong channel count
    with pytest.raises(ValueError):
        ops.fosls_apply(m.geom, u, mx, my, bc_values=(0.0,))
    with pytest.raises(ValueError):
        ops.fosls_apply(m.geom, u, mx, my, want_grad=False, want_sum=False)
    with pytest.raises(ValueError):
        ops.fosls_apply(m.geom, u, mx, my, fields=packed)
    with pytest.raises(ValueError):
        ops.fosls_apply(m.geom, fields=packed, want_grad=(True, False, False))
    with pytest.raises(ValueError):
        ops.fosls_apply(m.geom)


# ---------------------------------------------------------------------------------------------
# float64 restatement of the operator (include/diffnet_hip.h, dn_fosls_args)
# ---------------------------------------------------------------------------------------------
def fosls_np(u, mx, my, masks, vals, hx, hy, P, ngp, nu=1.0, f=None, f_gp=None, weights=(1.0, 1.0), fs=1.0, wscale=1.0, out_scale=1.0, *,
             tables=None, dtype=np.float64, scale=False):
    """u, mx, my: (ny, nx) float64; masks[k]: bool arrays or None; vals[k]: float or (ny, nx); nu: float or nodal (ny, nx); f: nodal
    (ny, nx) or None; f_gp: (G, nely, nelx), a float or None, g = jg * ngp + ig.  The formulas of the header, term by term, with the
    rule's truncated literals.  Returns (sum, (gu, gmx, gmy) each (ny, nx), (qx, qy, d) each (G, nely, nelx)).  dtype: the same
    statements in that type, inputs, tables and constants cast once at entry; tables: see test_strongform_host.elem_tables; scale: also
    returns (S_sum, (S_gu, S_gmx, S_gmy)), the magnitude field -- the same formulas with every input, table entry and constant replaced
    by its absolute value and every subtraction made an addition, after the Dirichlet substitutions; S_gu is 0 on the Dirichlet nodes."""
    from test_strongform_host import elem_tables
    dt = np.dtype(dtype).type
    ny, nx = np.shape(u)
    nely, nelx = (ny - 1) // P, (nx - 1) // P
    nb = P + 1
    G = ngp * ngp
    fixed = np.zeros((ny, nx), dtype=bool)
    for k in (0, 1):
        if masks[k] is not None:
            fixed |= np.asarray(masks[k], dtype=bool)

    def loc(jb, ib):
        return (slice(jb, jb + P * (nely - 1) + 1, P), slice(ib, ib + P * (nelx - 1) + 1, P))

    def run(A, minus):
        c = lambda x: A(np.asarray(x, dtype=dt))                                # noqa: E731
        Bt, Dt, _, Wt = (c(t) for t in elem_tables(P, ngp, tables, dt, wscale))
        wq, wd = (c(x)[()] for x in weights)
        fsc = c(fs)[()]
        sx, sy = dt(2) / dt(hx), dt(2) / dt(hy)
        ut, mxt, myt = c(u), c(mx), c(my)
        for k in (0, 1):                            # in order: where both hold, condition 2's value is the one used
            if masks[k] is not None:
                ut = np.where(masks[k], c(vals[k]), ut)
        total = dt(0)
        gu, gmx, gmy = (np.zeros((ny, nx), dtype=dt) for _ in range(3))
        qx_all, qy_all, d_all = (np.zeros((G, nely, nelx), dtype=dt) for _ in range(3))
        for jg in range(ngp):
            for ig in range(ngp):
                g, W = jg * ngp + ig, Wt[jg, ig]
                N = {(jb, ib): Bt[ig, ib] * Bt[jg, jb] for jb in range(nb) for ib in range(nb)}
                Nx = {(jb, ib): Dt[ig, ib] * sx * Bt[jg, jb] for jb in range(nb) for ib in range(nb)}
                Ny = {(jb, ib): Bt[ig, ib] * Dt[jg, jb] * sy for jb in range(nb) for ib in range(nb)}

                def at(t, tab):
                    return sum(tab[a] * t[loc(*a)] for a in tab)

                nug = at(c(nu), N) if np.ndim(nu) else c(float(nu))[()]
                if f is not None:
                    fg = at(c(f), N)
                elif f_gp is None or np.ndim(f_gp) == 0:
                    fg = np.full((nely, nelx), c(0.0 if f_gp is None else float(f_gp)), dtype=dt)
                else:
                    fg = c(f_gp)[g]
                qx = at(mxt, N) + minus * nug * at(ut, Nx)
                qy = at(myt, N) + minus * nug * at(ut, Ny)
                d = at(mxt, Nx) + at(myt, Ny) + fsc * fg
                qx_all[g], qy_all[g], d_all[g] = qx, qy, d
                total += W * np.sum(wq * (qx * qx + qy * qy) + wd * d * d)
                for a in N:
                    gu[loc(*a)] += minus * dt(2) * W * wq * nug * (qx * Nx[a] + qy * Ny[a])
                    gmx[loc(*a)] += dt(2) * W * (wq * qx * N[a] + wd * d * Nx[a])
                    gmy[loc(*a)] += dt(2) * W * (wq * qy * N[a] + wd * d * Ny[a])
        os_ = c(out_scale)
        grads = (np.where(fixed, dt(0), gu) * os_, gmx * os_, gmy * os_)
        assert all(x.dtype == dt for x in grads), [x.dtype for x in grads]         # numpy promotes silently
        return total, grads, (qx_all, qy_all, d_all)

    total, grads, parts = run(lambda x: x, dt(-1))
    if not scale:
        return total, grads, parts
    S_total, S_grads, _ = run(np.abs, dt(1))
    return total, grads, parts, (S_total, S_grads)


def fixture_case(z):
    kw = eval(str(z["kwargs"]))
    n, P = kw["domain_size"], kw["fem_basis_deg"]
    nel = (n - 1) // P
    h = 1.0 / nel
    return dict(masks=[z["mask1"][0, 0] != 0, z["mask2"][0, 0] != 0], vals=[float(z["v1"]), 0.0], hx=h, hy=h, P=P, ngp=kw["ngp_1d"],
                nu=z["inputs"][0, 0].astype(np.float64), f=z["forcing"][0, 0].astype(np.float64), weights=tuple(float(x) for x in z["weights"]),
                fs=float(z["fs"]), wscale=float(z["wscale"]), out_scale=1.0 / (nel * nel))


@pytest.mark.parametrize("name", FIXTURES)
def test_fosls_fixtures_agree_with_float64_restatement(name):
    z = np.load(os.path.join(GOLDEN, name))
    c = fixture_case(z)
    fl = z["fields"][0].astype(np.float64)
    total, grads, _ = fosls_np(fl[0], fl[1], fl[2], **c)
    loss = total * c["out_scale"]
    grad = np.stack(grads)
    ref = z["grad"][0]
    print(name, "loss rel", abs(loss - float(z["loss"])) / float(z["loss"]), "grad", np.abs(grad - ref).max() / np.abs(ref).max())
    lrt, grt, gar = FIXTURE_TOL[name]
    np.testing.assert_allclose(loss, float(z["loss"]), rtol=lrt)
    np.testing.assert_allclose(grad, ref, rtol=grt, atol=gar * np.abs(ref).max())


def test_fosls_fixtures_hold_what_they_should():
    for name in FIXTURES:
        z = np.load(os.path.join(GOLDEN, name))
        for k in ("kwargs", "fields", "inputs", "forcing", "mask1", "mask2", "v1", "weights", "fs", "wscale", "loss", "grad"):
            assert k in z.files, (name, k)
        kw = eval(str(z["kwargs"]))
        n = kw["domain_size"]
        assert z["fields"].shape == z["grad"].shape == z["inputs"].shape == (1, 3, n, n) and z["forcing"].shape == (1, 1, n, n)
        assert np.abs(z["fields"]).max() <= 1.0 and all(z["fields"][0, k].std() > 0.4 for k in range(3))     # order-one random, all channels
        m1, m2 = z["mask1"][0, 0] != 0, z["mask2"][0, 0] != 0
        # RectangleManufactured fixes the wall to 0 through condition 2 and leaves condition 1 (the source) empty: the Dirichlet set is
        # non-empty through mask2 alone, and mask1 is the dataset's (empty) channel as it is; condition 1 and the overlap rule are
        # covered by the central-difference test below and by the GPU tests
        assert m2.any() and (m1 | m2).any() and not (m1 | m2).all() and not m1.any()
        assert np.array_equal(m1, z["inputs"][0, 1] > 0.5) and np.array_equal(m2, z["inputs"][0, 2] > 0.5)
        assert float(z["v1"]) == 1.0 and tuple(z["weights"]) == (1.0, 1.0) and float(z["fs"]) == 1.0 and float(z["wscale"]) == 1.0
        g = z["grad"][0]
        assert np.all(g[0][m1 | m2] == 0.0)          # the reference's torch.where passes no gradient of u to a Dirichlet node ...
        assert np.all(g[0][~(m1 | m2)] != 0.0) and np.abs(g[1][m1 | m2]).min() > 0 and np.abs(g[2][m1 | m2]).min() > 0     # ... only
        assert np.isfinite(float(z["loss"])) and float(z["loss"]) > 0
    kws = [eval(str(np.load(os.path.join(GOLDEN, name))["kwargs"])) for name in FIXTURES]
    assert [(k["fem_basis_deg"], k["ngp_1d"], k["domain_size"]) for k in kws] == [(1, 2, 9), (1, 3, 9), (2, 3, 9), (3, 4, 10)]


@pytest.mark.parametrize("P,ngp,nx,ny", [(2, 3, 7, 5), (3, 4, 7, 4), (1, 2, 5, 4)])
def test_fosls_gradients_of_the_restatement_equal_central_differences(P, ngp, nx, ny):
    """float64 central differences of the sum with respect to every node of u, mx and my (the sum is quadratic in the fields, so the
    differences are exact up to rounding)"""
    rs = np.random.default_rng(15 + P)
    flds = [2 * rs.random((ny, nx)) - 1 for _ in range(3)]
    m1, m2 = rs.random((ny, nx)) < 0.2, rs.random((ny, nx)) < 0.2
    m1[0, 0] = m2[0, 0] = True                      # both conditions on one node at least
    m1[-1, -1] = m2[-1, -1] = False
    c = dict(masks=[m1, m2], vals=[2 * rs.random((ny, nx)) - 1, 0.3], hx=0.2, hy=0.25, P=P, ngp=ngp, nu=0.5 + rs.random((ny, nx)),
             f=rs.random((ny, nx)) - 0.5, weights=(0.7, 1.3), fs=0.9, wscale=0.8, out_scale=0.37)
    _, grads, _ = fosls_np(*flds, **c)
    assert all(np.abs(g).max() > 1e-2 for g in grads) and np.all(grads[0][m1 | m2] == 0.0) and (m1 & m2).any()
    eps = 1e-4
    for k in range(3):
        fd = np.zeros((ny, nx))
        for j in range(ny):
            for i in range(nx):
                up, um = [x.copy() for x in flds], [x.copy() for x in flds]
                up[k][j, i] += eps
                um[k][j, i] -= eps
                fd[j, i] = c["out_scale"] * (fosls_np(*up, **c)[0] - fosls_np(*um, **c)[0]) / (2 * eps)
        np.testing.assert_allclose(grads[k], fd, rtol=0, atol=1e-7 * np.abs(fd).max(), err_msg=f"field {k}")
    # with a constant coefficient and Gauss-point forcing
    c2 = dict(c, nu=0.8, f=None, f_gp=rs.random((ngp * ngp, (ny - 1) // P, (nx - 1) // P)))
    _, grads2, _ = fosls_np(*flds, **c2)
    j, i = np.argwhere(~(m1 | m2))[0]
    for k in range(3):
        up, um = [x.copy() for x in flds], [x.copy() for x in flds]
        up[k][j, i] += eps
        um[k][j, i] -= eps
        fd2 = c["out_scale"] * (fosls_np(*up, **c2)[0] - fosls_np(*um, **c2)[0]) / (2 * eps)
        np.testing.assert_allclose(grads2[k][j, i], fd2, rtol=0, atol=1e-7 * np.abs(grads2[k]).max())
