"""CPU checks of the fused 2-D eikonal weak-form residual (dn_eikonal_apply, csrc/eikonal.hip): the C ABI and its ctypes binding agree and
the library validates its arguments before any launch; the reference fixtures (tests/golden/loss_eikonal_*.npz, written by
tools/gen_golden_eikonal.py from the reference script's own loss body) agree with a float64 torch restatement of the operator kept here
(the script's spelling, differentiated by autograd), every one of its three terms is visible in the fixtures' loss, and the hand-derived
pullback of the kernel's VJP mode (include/diffnet_hip.h), restated in numpy, equals the restatement's autograd VJP."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_stokes_host import header_struct
from test_transport_host import GRAD_AREL, GRAD_RTOL, LOSS_RTOL

FIXTURES = ["loss_eikonal_fixedbc_n17.npz", "loss_eikonal_fixedbc_n9_g3.npz"]


def ek_mesh(n=13, deg=2, ngp=3, B=2, ny=None):
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    gx, gw = gauss_rule(ngp)
    ny = n if ny is None else ny
    return FemGeometry(2, (n, ny), (1 / (n - 1), 1 / (ny - 1)), deg, ngp, gx, gw).mesh_struct(B)


def workspace_formula(m):
    """include/diffnet_hip.h, dn_eikonal_args: 4160 + 16 * chunks * nely * B"""
    Q, nely = (m.nx - 1) // m.degree + 1, (m.ny - 1) // m.degree
    chunks = 1 if Q <= 64 else -(-(Q - 1) // 63)
    return 4160 + 16 * chunks * nely * m.batch


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_eikonal_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    for s in ("dn_eikonal_workspace_bytes", "dn_eikonal_apply"):
        assert hasattr(h, s) and s in _lib.SYMBOLS, s
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    got = [(n, getattr(t, "_length_", 1)) for n, t in _lib.DnEikonalArgs._fields_]
    assert got == header_struct("dn_eikonal_args")
    # the C layout (x86-64): one pointer, 2 x 40 bytes of conditions, 2 pointers, a word + 4 floats + a word, 8 pointers, one int64
    A = _lib.DnEikonalArgs
    assert C.sizeof(A) == 192 and A.bc.offset == 8 and A.f.offset == 88 and A.vjp.offset == 124 and A.cot.offset == 128 and A.out.offset == 152


def test_eikonal_workspace_bytes_and_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    for deg, ngp, n in ((1, 2, 9), (1, 3, 9), (1, 4, 9), (2, 3, 9), (2, 4, 9), (3, 3, 10), (3, 4, 10)):
        m = ek_mesh(n, deg, ngp)
        got = h.dn_eikonal_workspace_bytes(C.byref(m))
        assert got > 0 and got == workspace_formula(m), (deg, ngp)
    for n, deg, B, ny in ((257, 2, 8, None), (65, 1, 3, 9), (64, 1, 1, 64), (193, 3, 2, 10), (512, 1, 16, 512)):
        m = ek_mesh(n, deg, 3, B=B, ny=ny)
        assert h.dn_eikonal_workspace_bytes(C.byref(m)) == workspace_formula(m), (n, deg, B)
    for field, bad in (("nsd", 3), ("nx", 1), ("ny", 0), ("batch", 0), ("ngp", 5), ("ngp", 1), ("ngp", 2), ("degree", 4), ("nx", 12)):
        m = ek_mesh()
        setattr(m, field, bad)
        assert h.dn_eikonal_workspace_bytes(C.byref(m)) == -1, field
    m = ek_mesh()
    # every pointer below is a small odd number: a check that came after a launch or a dereference would not return
    assert h.dn_eikonal_apply(C.byref(m), None, None) == -1
    assert h.dn_eikonal_apply(None, None, None) == -1
    a = _lib.DnEikonalArgs()                        # a NULL u
    a.out = 64
    assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -1
    a.out = None
    a.u = 16                                        # a field but no output at all
    assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -1
    for name in ("sumsq", "norm"):
        setattr(a, name, 128)                       # a sum without a workspace
        assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -3, name
        a.workspace, a.workspace_bytes = 256, 64    # ... or with one that is too small
        assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -3, name
        a.workspace_bytes = h.dn_eikonal_workspace_bytes(C.byref(m)) - 1
        assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -3, name
        setattr(a, name, None)
        a.workspace, a.workspace_bytes = None, 0
    a.out = 64
    for deg, ngp in ((2, 2), (3, 2), (4, 3), (0, 2), (1, 5), (1, 1)):          # a degree / ngp combination outside the domain
        mm = ek_mesh()
        mm.degree, mm.ngp, mm.nx, mm.ny = deg, ngp, 13, 13
        assert h.dn_eikonal_apply(C.byref(mm), C.byref(a), None) == -2, (deg, ngp)
    mm = ek_mesh()
    mm.nx = 12                                      # (n - 1) % degree != 0
    assert h.dn_eikonal_apply(C.byref(mm), C.byref(a), None) == -1
    mm = ek_mesh()
    mm.nsd = 3
    assert h.dn_eikonal_apply(C.byref(mm), C.byref(a), None) == -1
    # packed and box masks
    for k in (0, 1):
        for kind in (_lib.MASK_BITS, _lib.MASK_BOX):
            a.bc[k].mask_kind = kind
            assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -2, (k, kind)
            a.bc[k].mask, a.bc[k].box_faces = 512, 15
            assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -2, (k, kind)
            a.bc[k].mask, a.bc[k].box_faces = None, 0
        a.bc[k].mask_kind = 7
        assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -1
        a.bc[k].mask_kind = 0
        a.bc[k].field = 120                         # a value field without its mask
        assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -1
        a.bc[k].field = None
        for flag in ("mask_batched", "field_batched"):
            setattr(a.bc[k], flag, 2)
            assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -1, flag
            setattr(a.bc[k], flag, 0)
    for flag, bad in (("f_batched", 2), ("vjp", 2), ("vjp", -1)):
        setattr(a, flag, bad)
        assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -1, flag
        setattr(a, flag, 0)
    a.f, a.f_gp = 32, 48                            # nodal and Gauss-point forcing at once
    assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -1
    a.f, a.f_gp = None, None
    a.vjp = 1                                       # a VJP without its cotangent
    assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -1
    a.cot = 80
    a.in_den = 96                                   # in_den without in_num
    assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -1
    a.vjp, a.cot, a.in_den = 0, None, None
    a.in_num = 96                                   # in_num outside the VJP
    assert h.dn_eikonal_apply(C.byref(m), C.byref(a), None) == -1


def test_eikonal_ops_refuse_cpu_tensors_and_bad_arguments():
    from diffnet_amd import DiffNet2DFEM, ops
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd import eikonal as ek
    assert ek.eikonal_coefficients(0.25) == dict(tau=0.25, sq=1.25)
    m = DiffNet2DFEM(None, domain_size=9, fem_basis_deg=2)
    u = torch.zeros((1, 1, 9, 9))
    with pytest.raises(DiffNetHipError):
        ops.eikonal_apply(m.geom, u)
    for fn in (ek.eikonal_residual, ek.eikonal_loss, ek.eikonal_loss_and_grad):
        with pytest.raises(DiffNetHipError):
            fn(m, u, tau=0.25)
    for fn in (ek.eikonal_loss, ek.eikonal_loss_and_grad):
        with pytest.raises(ValueError):
            fn(m, u, kind="max")
    with pytest.raises(ValueError):
        ek.eikonal_loss(m, u, bc_values=(0.0,))
    with pytest.raises(ValueError):
        ops.eikonal_apply(m.geom, u, bc_values=(0.0,))
    with pytest.raises(ValueError):
        ops.eikonal_apply(m.geom, u, want_out=False)
    with pytest.raises(ValueError):
        ops.eikonal_apply(m.geom, u, in_num=torch.ones(1))          # a scale without a cotangent
    with pytest.raises(ValueError):
        ops.eikonal_apply(m.geom, u, cot=u, in_den=torch.ones(1))   # in_den without in_num


# ---------------------------------------------------------------------------------------------
# float64 restatement of the operator, in the scripts' spelling (torch, differentiable) and the pullback by hand (numpy)
# ---------------------------------------------------------------------------------------------
def _loc(P, nely, nelx, jb, ib):
    return (slice(jb, jb + P * (nely - 1) + 1, P), slice(ib, ib + P * (nelx - 1) + 1, P))


def _tables_kw(P, ngp, hx, hy, wscale, tables, npd):
    """(N, dN, W[jg][ig], 2 / hx, 2 / hy) in the numpy type npd; tables: see test_strongform_host.elem_tables"""
    from test_strongform_host import elem_tables
    Bt, Dt, _, Wt = elem_tables(P, ngp, tables, npd, wscale)
    return Bt, Dt, Wt, npd(2) / npd(hx), npd(2) / npd(hy)


def eikonal_t64(u, hx, hy, P, ngp, tau, sq=None, f=1.0, wscale=None, masks=(None, None), vals=(0.0, 0.0), drop=None, *, tables=None,
                dtype=torch.float64, scale=False):
    """R (ny, nx) of the header's formula from u (ny, nx), a float64 torch tensor (differentiable): the scripts' sum over the Gauss points of
    JxW (tau u (dN_x u_x + dN_y u_y) + sq N (u_x^2 + u_y^2) - N f), assembled, zero on the Dirichlet nodes.  f: a float, a nodal (ny, nx)
    tensor or a Gauss-point (G, nely, nelx) one, g = jg * ngp + ig.  drop: "stab" | "sq" | "rhs" leaves that term out.  dtype: the same
    statements in that torch type, inputs, tables and constants cast once at entry; tables: see test_strongform_host.elem_tables; scale:
    returns (R, S), S the magnitude field -- the same formula with every input, table entry and constant replaced by its absolute value
    and the subtraction made an addition, after the Dirichlet substitutions; 0 on the Dirichlet nodes."""
    npd = np.float32 if dtype == torch.float32 else np.float64
    sq = 1.0 + tau if sq is None else sq
    wscale = (0.5 * hx) * (0.5 * hy) if wscale is None else wscale
    ny, nx = u.shape
    nely, nelx = (ny - 1) // P, (nx - 1) // P
    nb = P + 1
    fixed = torch.zeros((ny, nx), dtype=torch.bool)
    for k in (0, 1):
        if masks[k] is not None:
            fixed |= torch.as_tensor(masks[k], dtype=torch.bool)

    def run(A, minus):
        Bt, Dt, Wt, sx, sy = (A(t) for t in _tables_kw(P, ngp, hx, hy, wscale, tables, npd))
        c = lambda x: A(x.to(dtype)) if isinstance(x, torch.Tensor) else float(A(npd(x)))            # noqa: E731
        tau_, sq_ = c(tau), c(sq)
        ut = c(u)
        for k in (0, 1):
            if masks[k] is not None:
                mk = torch.as_tensor(masks[k], dtype=torch.bool)
                v = c(vals[k]) if isinstance(vals[k], torch.Tensor) else torch.full_like(ut, c(vals[k]))
                ut = torch.where(mk, v, ut)
        out = torch.zeros((ny, nx), dtype=dtype)
        for jg in range(ngp):
            for ig in range(ngp):
                W = float(Wt[jg, ig])
                N = {(jb, ib): float(Bt[ig, ib] * Bt[jg, jb]) for jb in range(nb) for ib in range(nb)}
                Nx = {(jb, ib): float(Dt[ig, ib] * sx * Bt[jg, jb]) for jb in range(nb) for ib in range(nb)}
                Ny = {(jb, ib): float(Bt[ig, ib] * Dt[jg, jb] * sy) for jb in range(nb) for ib in range(nb)}

                def at(t, tab):
                    return sum(tab[a] * t[_loc(P, nely, nelx, *a)] for a in tab)

                ug, ux, uy = at(ut, N), at(ut, Nx), at(ut, Ny)
                if isinstance(f, torch.Tensor) and f.dim() == 3:
                    fg = c(f)[jg * ngp + ig]
                elif isinstance(f, torch.Tensor):
                    fg = at(c(f), N)
                else:
                    fg = torch.full_like(ug, c(f))
                for a in N:
                    t = 0.0
                    if drop != "stab":
                        t = t + tau_ * ug * (Nx[a] * ux + Ny[a] * uy)
                    if drop != "sq":
                        t = t + sq_ * N[a] * (ux ** 2 + uy ** 2)
                    if drop != "rhs":
                        t = t + minus * N[a] * fg
                    sl = _loc(P, nely, nelx, *a)
                    out[sl] = out[sl] + W * t
        assert out.dtype == dtype, out.dtype
        return torch.where(fixed, torch.zeros_like(out), out)

    R = run(lambda x: x, -1.0)
    if not scale:
        return R
    with torch.no_grad():
        return R, run(abs, 1.0)


def eikonal_pullback_np(u, cot, hx, hy, P, ngp, tau, sq=None, wscale=None, masks=(None, None), vals=(0.0, 0.0), *, tables=None,
                        dtype=np.float64, scale=False):
    """The VJP of the header: with the cotangent (zero on the Dirichlet nodes) evaluated like a field (L, L_x, L_y),
    A' = tau (L_x u_x + L_y u_y), B' = 2 sq L u_x + tau u L_x, C' = 2 sq L u_y + tau u L_y on N | Nx | Ny, assembled, zero on the Dirichlet
    nodes.  dtype: the same statements in that type, inputs, tables and constants cast once at entry; tables: see
    test_strongform_host.elem_tables; scale: returns (out, S), S the magnitude field -- the same formula with every input, table entry
    and constant replaced by its absolute value (there is no subtraction), after the Dirichlet substitutions; 0 on the Dirichlet nodes."""
    dt = np.dtype(dtype).type
    sq = 1.0 + tau if sq is None else sq
    wscale = (0.5 * hx) * (0.5 * hy) if wscale is None else wscale
    ny, nx = np.shape(u)
    nely, nelx = (ny - 1) // P, (nx - 1) // P
    nb = P + 1
    fixed = np.zeros((ny, nx), dtype=bool)
    for k in (0, 1):
        if masks[k] is not None:
            fixed |= np.asarray(masks[k], dtype=bool)

    def run(A):
        c = lambda x: A(np.asarray(x, dtype=dt))                                # noqa: E731
        Bt, Dt, Wt, sx, sy = (A(t) for t in _tables_kw(P, ngp, hx, hy, wscale, tables, dt))
        tau_, sq_ = c(tau)[()], c(sq)[()]
        ut = c(u)
        for k in (0, 1):
            if masks[k] is not None:
                ut = np.where(masks[k], c(vals[k]), ut)
        lt = np.where(fixed, dt(0), c(cot))
        out = np.zeros((ny, nx), dtype=dt)
        for jg in range(ngp):
            for ig in range(ngp):
                W = Wt[jg, ig]
                N = {(jb, ib): Bt[ig, ib] * Bt[jg, jb] for jb in range(nb) for ib in range(nb)}
                Nx = {(jb, ib): Dt[ig, ib] * sx * Bt[jg, jb] for jb in range(nb) for ib in range(nb)}
                Ny = {(jb, ib): Bt[ig, ib] * Dt[jg, jb] * sy for jb in range(nb) for ib in range(nb)}

                def at(t, tab):
                    return sum(tab[a] * t[_loc(P, nely, nelx, *a)] for a in tab)

                ug, ux, uy = at(ut, N), at(ut, Nx), at(ut, Ny)
                L, Lx, Ly = at(lt, N), at(lt, Nx), at(lt, Ny)
                Ac = tau_ * (Lx * ux + Ly * uy)
                Bc = dt(2) * sq_ * L * ux + tau_ * ug * Lx
                Cc = dt(2) * sq_ * L * uy + tau_ * ug * Ly
                for a in N:
                    out[_loc(P, nely, nelx, *a)] += W * (N[a] * Ac + Nx[a] * Bc + Ny[a] * Cc)
        assert out.dtype == dt, out.dtype                                          # numpy promotes silently
        return np.where(fixed, dt(0), out)

    out = run(lambda x: x)
    return (out, run(np.abs)) if scale else out


def fixture_case(z):
    kw = eval(str(z["kwargs"]))
    n = kw["domain_size"]
    h = 1.0 / (n - 1)
    return dict(hx=h, hy=h, P=1, ngp=kw.get("ngp_1d", 2), tau=float(z["tau"]), sq=float(z["sq"]), wscale=float(z["wscale"]))


def fixture_loss_and_grad(z, drop=None):
    """(||R||_F + the fixture's point terms, the gradient of ||R||_F, R) of the restatement on the fixture's u"""
    u = torch.tensor(z["u"][0, 0].astype(np.float64), requires_grad=True)
    R = eikonal_t64(u, drop=drop, **fixture_case(z))
    nrm = torch.norm(R)
    g, = torch.autograd.grad(nrm, u)
    return float(nrm.detach()) + float(z["point_terms"]), g.numpy(), R.detach().numpy()


@pytest.mark.parametrize("name", FIXTURES)
def test_eikonal_fixtures_agree_with_float64_restatement(name):
    z = np.load(os.path.join(GOLDEN, name))
    for k in ("kwargs", "script", "u", "pc", "tau", "sq", "wscale", "R1", "point_terms", "loss", "grad"):
        assert k in z.files, (name, k)
    assert float(z["tau"]) == 0.25 and float(z["sq"]) == 1.25 and float(z["point_terms"]) in (1.0, 2.0)
    loss, grad, R = fixture_loss_and_grad(z)
    ref = z["grad"][0, 0]
    print(name, "loss rel", abs(loss - float(z["loss"])) / float(z["loss"]), "grad", np.abs(grad - ref).max() / np.abs(ref).max(),
          "R1", np.abs(R - z["R1"]).max() / np.abs(z["R1"]).max())
    np.testing.assert_allclose(loss, float(z["loss"]), rtol=LOSS_RTOL)
    np.testing.assert_allclose(grad, ref, rtol=GRAD_RTOL, atol=GRAD_AREL * np.abs(ref).max())
    np.testing.assert_allclose(R, z["R1"], rtol=GRAD_RTOL, atol=GRAD_AREL * np.abs(z["R1"]).max())
    # the neutral point: u is exactly 0 on the nodes around its element, and |grad u| = O(1) elsewhere
    n = z["u"].shape[-1]
    k = int(float(z["pc"][0]) * (n - 1))
    assert np.all(z["u"][0, 0, k:k + 2, k:k + 2] == 0.0) and 0.1 < np.abs(z["u"]).max() < 1.0


@pytest.mark.parametrize("name", FIXTURES)
def test_eikonal_every_term_is_visible_in_the_fixtures(name):
    z = np.load(os.path.join(GOLDEN, name))
    ref = float(z["loss"])
    for drop in ("stab", "sq", "rhs"):
        loss, _, _ = fixture_loss_and_grad(z, drop=drop)
        print(name, "without", drop, "loss moves by", abs(loss - ref) / ref, "relative")
        assert abs(loss - ref) >= 100 * LOSS_RTOL * ref, (name, drop)


@pytest.mark.parametrize("P,ngp,nx,ny", [(1, 2, 7, 6), (2, 3, 7, 5), (3, 4, 7, 4)])
def test_eikonal_pullback_by_hand_equals_autograd_of_the_restatement(P, ngp, nx, ny):
    rs = np.random.default_rng(5 + P)
    m1, m2 = rs.random((ny, nx)) < 0.2, rs.random((ny, nx)) < 0.2
    m1[0, 0] = m2[0, 0] = True                      # the two conditions overlap
    m1[1, 1], m2[1, 1] = False, False
    v1, v2 = 2 * rs.random((ny, nx)) - 1, 2 * rs.random((ny, nx)) - 1
    u0, cot = 2 * rs.random((ny, nx)) - 1, 2 * rs.random((ny, nx)) - 1
    c = dict(hx=0.2, hy=0.25, P=P, ngp=ngp, tau=0.25, sq=1.4, wscale=0.8)
    for masks, vals in (((None, None), (0.0, 0.0)), ((m1, m2), (v1, v2))):
        u = torch.tensor(u0, requires_grad=True)
        R = eikonal_t64(u, f=torch.tensor(rs.random((ny, nx))), masks=masks, vals=tuple(torch.as_tensor(v, dtype=torch.float64) for v in vals), **c)
        g, = torch.autograd.grad(R, u, torch.tensor(cot))
        mine = eikonal_pullback_np(u0, cot, masks=masks, vals=vals, **c)
        assert np.abs(g.numpy()).max() > 1e-2
        np.testing.assert_allclose(mine, g.numpy(), rtol=0, atol=1e-12 * np.abs(g.numpy()).max())
        if masks[0] is not None:
            assert np.all(mine[m1 | m2] == 0.0) and np.all(R.detach().numpy()[m1 | m2] == 0.0)
