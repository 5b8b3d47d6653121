"""CPU checks of the fused 2-D scalar transport (SUPG) residual (dn_transport_apply, csrc/transport.hip): the C ABI and its ctypes
binding agree and the library validates its arguments before any launch; the reference fixtures (tests/golden/loss_transport_*.npz, written
by tools/gen_golden_transport.py from the reference scripts' own `loss` bodies) agree with a float64 torch restatement of the operator kept
here, loss and gradient; every term of the operator is visible in the fixture it belongs to; and the pointwise pullback the VJP launch
implements, restated in numpy, equals the restatement's autograd VJP."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_ns_host import _np_type, _q1_point_tables
from test_stokes_host import header_struct, q1_tables, stokes_mesh

FIXTURES = ["loss_transport_advdiff_n17.npz", "loss_transport_stheat_n33_g3.npz", "loss_transport_allencahn_n17.npz",
            "loss_transport_allencahn_n9_g4.npz"]
# DESIGN.md section 2, fp32 references: scalar losses rtol 1e-5, gradients rtol 1e-4 / atol 1e-4 max|ref|
LOSS_RTOL, GRAD_RTOL, GRAD_AREL = 1e-5, 1e-4, 1e-4


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_transport_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    for s in ("dn_transport_workspace_bytes", "dn_transport_apply"):
        assert hasattr(h, s) and s in _lib.SYMBOLS, s
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    got = [(n, getattr(t, "_length_", 1)) for n, t in _lib.DnTransportArgs._fields_]
    assert got == header_struct("dn_transport_args")
    names = [n for n, _ in got]
    for n in ("u", "nu", "nu_batched", "bc_mask", "mask_is_u8", "mask_batched", "bc_field", "bc_field_batched", "bc_value", "r_first_wins",
              "f_gp", "f_batched", "f_value", "adv", "kappa", "tau", "react", "wscale", "vjp", "cot", "out", "sumsq", "norm", "in_num",
              "in_den", "workspace", "workspace_bytes"):
        assert n in names, n
    assert C.sizeof(_lib.DnTransportArgs) == 216 and _lib.DnTransportArgs.cot.offset == 152          # the C layout (x86-64)


def test_transport_workspace_bytes_and_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    for ngp in (2, 3, 4):
        assert h.dn_transport_workspace_bytes(C.byref(stokes_mesh(ngp=ngp))) > 0
    big = h.dn_transport_workspace_bytes(C.byref(stokes_mesh(n=2049, B=8, ny=1025)))
    assert big > 64 * 65 and (big - 64 * 65) % 8 == 0              # the header + one double per workgroup
    for field, bad in (("nsd", 3), ("degree", 2), ("nx", 1), ("ny", 0), ("batch", 0), ("ngp", 5), ("ngp", 1)):
        m = stokes_mesh()
        setattr(m, field, bad)
        assert h.dn_transport_workspace_bytes(C.byref(m)) == -1, field
    m = stokes_mesh()
    assert h.dn_transport_apply(C.byref(m), None, None) == -1
    assert h.dn_transport_apply(None, None, None) == -1
    a = _lib.DnTransportArgs()                      # no field
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -1
    a.u = 16                                        # a field but no output: rejected before anything touches the pointers
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -1
    a.out = 64
    a.in_den = 88                                   # in_den without in_num
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -1
    a.in_num = 80                                   # both, but not in the VJP mode
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -1
    a.in_den = None                                 # in_num alone, still not in the VJP mode
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -1
    a.in_num = None
    a.vjp = 1                                       # a VJP without its cotangent
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -1
    a.vjp = 2
    a.cot = 96
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -1
    a.vjp = 0
    for flag in ("r_first_wins", "nu_batched", "f_batched"):
        setattr(a, flag, 2)
        assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -1, flag
        setattr(a, flag, 0)
    for arr in ("mask_is_u8", "mask_batched", "bc_field_batched"):
        getattr(a, arr)[1] = 2
        assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -1, arr
        getattr(a, arr)[1] = 0
    a.bc_field[1] = 120                             # a value field without its mask
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -1
    a.bc_field[1] = None
    a.norm = 128                                    # a reduction without a workspace
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -3
    a.workspace, a.workspace_bytes = 256, 64        # ... or with one that is too small
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -3
    m.degree = 2
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -2
    m.degree, m.nsd = 1, 3
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -2
    m.nsd, m.ngp = 2, 5
    assert h.dn_transport_apply(C.byref(m), C.byref(a), None) == -2


def test_transport_ops_refuse_cpu_tensors_and_unsupported_meshes():
    from diffnet_amd import DiffNet2DFEM, ops
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd.transport import transport_loss, transport_residual
    m = DiffNet2DFEM(None, domain_size=9)
    u = torch.zeros((1, 1, 9, 9))
    with pytest.raises(DiffNetHipError):
        ops.transport_apply(m.geom, u)
    with pytest.raises(DiffNetHipError):
        transport_residual(m, u)
    with pytest.raises(DiffNetHipError):
        transport_loss(m, u, adv=(1.0, 0.0))
    m2 = DiffNet2DFEM(None, domain_size=9, fem_basis_deg=2)
    with pytest.raises(DiffNetHipError):
        ops.transport_apply(m2.geom, u)
    with pytest.raises(ValueError):
        ops.transport_apply(m.geom, u, bc_values=(0.0,))
    with pytest.raises(ValueError):
        ops.transport_apply(m.geom, u, react=(0.0, 0.0))
    with pytest.raises(ValueError):
        transport_loss(m, u, kind="max")


def test_transport_coefficient_helpers_return_the_scripts_values():
    from diffnet_amd import DiffNet2DFEM
    from diffnet_amd.transport import advdiff_coefficients, allen_cahn_coefficients, space_time_heat_coefficients
    m = DiffNet2DFEM(None, domain_size=17)
    h = 1.0 / 16
    a = (np.cos(np.pi / 6), np.sin(np.pi / 6))
    adv, kap, tau, react = advdiff_coefficients(m, a, 1e-2)
    assert adv == a and kap == (1e-2, 1e-2) and react == (0.0,) * 4
    np.testing.assert_allclose(tau, 1.0 / (2.0 / h + 4e-2 / h ** 2), rtol=1e-12)
    assert space_time_heat_coefficients(m, 0.3) == ((0.0, 1.0), (0.3, 0.0), h / 2, (0.0,) * 4)
    adv, kap, tau, react = allen_cahn_coefficients(A=2.0, Cn=0.1, D=3.0, k=0.5)
    assert adv == (0.0, 1.0) and tau == 0.0
    np.testing.assert_allclose(kap, (0.03, 0.03), rtol=1e-12)
    np.testing.assert_allclose(react, (-4.5, 36.0, -108.0, 72.0), rtol=1e-12)


# ---------------------------------------------------------------------------------------------
# float64 restatement of the operator (include/diffnet_hip.h, dn_transport_args)
# ---------------------------------------------------------------------------------------------
def _tables(ngp, hx, hy, ig, jg, tables=None, dt=np.float64, as_float=False):
    """N_a, Nx_a, Ny_a of the four local nodes at Gauss point (ig, jg), computed in the type `dt` (as Python floats for torch)"""
    N, dN, _ = (np.asarray(t, dtype=dt) for t in (q1_tables(ngp) if tables is None else tables))
    return _q1_point_tables(N, dN, dt(2) / dt(hx), dt(2) / dt(hy), ig, jg, as_float=as_float)


def _place(t, ly, lx):
    """an element array (nely, nelx) of local node (ly, lx) at its nodes (ny, nx)"""
    return torch.nn.functional.pad(t, (lx, 1 - lx, ly, 1 - ly))


def transport_torch(u, nu, masks, vals, f, adv, kappa, tau, react, J, hx, hy, ngp, first, *, scale=False, dtype=torch.float64, tables=None):
    """u: (ny, nx) float64 tensor; nu: (ny, nx) or None; masks[k]: bool arrays or None; vals[k]: float or (ny, nx); f: (G, nely, nelx) or a
    float, g = jg * ngp + ig.  The formulas of the header, term by term.  Returns R (ny, nx), differentiable wrt u.
    dtype: the same statements in that type, with tables, constants and inputs cast once at entry; tables: the 1-D (N, dN, w) to use in
    place of q1_tables(ngp); scale: also returns S, the sum of |w_g t| over the placed terms that make up the node's value (0 on the
    Dirichlet nodes)."""
    dt = _np_type(dtype)
    w = np.asarray((q1_tables(ngp) if tables is None else tables)[2], dtype=dt)
    u = u.to(dtype)
    # tau adv[k]: one product (float64: of the caller's own scalars, as before there were types to choose)
    tadv = [float(tau * a) if dt is np.float64 else float(dt(tau) * dt(a)) for a in adv]
    adv, kappa, react, J = [float(dt(x)) for x in adv], [float(dt(x)) for x in kappa], [float(dt(x)) for x in react], dt(J)
    ny, nx = u.shape
    masks = [None if m is None else torch.as_tensor(m) for m in masks]
    vals = [torch.as_tensor(x, dtype=dtype).expand(ny, nx) for x in vals]
    f = torch.as_tensor(f, dtype=dtype)
    f = f.expand(ngp * ngp, ny - 1, nx - 1) if f.dim() == 0 else f
    ut = u
    for k in (0, 1):                                  # condition 2 last: it wins on u
        if masks[k] is not None:
            ut = torch.where(masks[k], vals[k], ut)
    nut = torch.ones((ny, nx), dtype=dtype) if nu is None else torch.as_tensor(nu, dtype=dtype)
    R = torch.zeros((ny, nx), dtype=dtype)
    S = torch.zeros((ny, nx), dtype=dtype)
    fixed = torch.zeros((ny, nx), dtype=torch.bool)
    for jg in range(ngp):
        for ig in range(ngp):
            g, wg = jg * ngp + ig, float(J * w[ig] * w[jg])
            Na, Nxa, Nya = _tables(ngp, hx, hy, ig, jg, tables, dt, as_float=True)

            def at(t, tab):
                return sum(tab[ly, lx] * t[ly:ny - 1 + ly, lx:nx - 1 + lx] for ly in (0, 1) for lx in (0, 1))

            ug, ux, uy, nug = at(ut, Na), at(ut, Nxa), at(ut, Nya), at(nut, Na)
            a_ = adv[0] * ux + adv[1] * uy
            A = a_ + react[0] + react[1] * ug + react[2] * ug ** 2 + react[3] * ug ** 3 - f[g]
            B = kappa[0] * nug * ux + tadv[0] * (a_ - f[g])
            Cc = kappa[1] * nug * uy + tadv[1] * (a_ - f[g])
            for (ly, lx), n_ in Na.items():
                t = wg * (n_ * A + Nxa[ly, lx] * B + Nya[ly, lx] * Cc)
                R = R + _place(t, ly, lx)
                if scale:
                    S = S + _place(t.detach().abs(), ly, lx)
    for k in ((1, 0) if first else (0, 1)):           # the condition applied last wins on the rows of R
        if masks[k] is not None:
            R = torch.where(masks[k], vals[k], R)
            fixed = fixed | masks[k]
    assert R.dtype == dtype, R.dtype
    return (R, torch.where(fixed, torch.zeros_like(S), S)) if scale else R


def fixture_case(z):
    kw = eval(str(z["kwargs"]))
    n = kw["domain_size"]
    h = 1.0 / (n - 1)
    inp = z["inputs"].astype(np.float64)
    v1 = z["v1"].astype(np.float64)
    return dict(nu=inp[0, 0] if int(z["uses_nu"]) else None, masks=[inp[0, 1] > 0.5, inp[0, 2] > 0.5], vals=[v1 if v1.ndim else float(v1), 0.0],
                f=z["f_gp"].astype(np.float64), adv=tuple(z["adv"]), kappa=tuple(z["kappa"]), tau=float(z["tau"]), react=tuple(z["react"]),
                J=float(z["wscale"]), hx=h, hy=h, ngp=kw.get("ngp_1d", 2), first=bool(z["r_first_wins"]))


def loss_and_grad(u, c):
    ut = torch.tensor(u, dtype=torch.float64, requires_grad=True)
    loss = (transport_torch(ut, **c) ** 2).sum()
    g, = torch.autograd.grad(loss, ut)
    return float(loss.detach()), g.numpy()


@pytest.mark.parametrize("name", FIXTURES)
def test_transport_fixtures_agree_with_float64_restatement(name):
    z = np.load(os.path.join(GOLDEN, name))
    loss, grad = loss_and_grad(z["u"][0, 0], fixture_case(z))
    ref = z["grad"][0, 0]
    print(name, "loss rel", abs(loss - float(z["loss"])) / float(z["loss"]), "grad", np.abs(grad - ref).max() / np.abs(ref).max())
    np.testing.assert_allclose(loss, float(z["loss"]), rtol=LOSS_RTOL)
    np.testing.assert_allclose(grad, ref, rtol=GRAD_RTOL, atol=GRAD_AREL * np.abs(ref).max())


def _variants(c):
    """the fixture with each non-zero ingredient removed in turn"""
    out = []
    if any(c["adv"]):
        out.append(("adv", dict(c, adv=(0.0, 0.0))))
    for k in (0, 1):
        if c["kappa"][k]:
            out.append((f"kappa[{k}]", dict(c, kappa=tuple(0.0 if i == k else x for i, x in enumerate(c["kappa"])))))
    if c["tau"]:
        out.append(("tau", dict(c, tau=0.0)))
    for k in range(4):
        if c["react"][k]:
            out.append((f"react[{k}]", dict(c, react=tuple(0.0 if i == k else x for i, x in enumerate(c["react"])))))
    if c["nu"] is not None:
        out.append(("nu", dict(c, nu=None)))
    if np.abs(c["f"]).max() > 0:
        out.append(("f", dict(c, f=0.0)))
    if (c["masks"][0] & c["masks"][1]).any():
        out.append(("r_first_wins", dict(c, first=not c["first"])))
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_transport_every_term_is_visible_in_its_fixture(name):
    """Removing any one ingredient moves the loss or the gradient by at least 100 x the tolerance the fixture is compared under."""
    z = np.load(os.path.join(GOLDEN, name))
    c = fixture_case(z)
    u = z["u"][0, 0]
    loss, grad = loss_and_grad(u, c)
    names = [n for n, _ in _variants(c)]
    assert "f" in names and ("adv" in names)
    if "advdiff" in name:
        assert {"kappa[0]", "kappa[1]", "tau", "nu"} <= set(names)
    if "stheat" in name:
        assert {"kappa[0]", "tau", "r_first_wins"} <= set(names)
    if "allencahn" in name:
        assert {"kappa[0]", "kappa[1]", "react[0]", "react[1]", "react[2]", "react[3]"} <= set(names)
    for what, cv in _variants(c):
        l2, g2 = loss_and_grad(u, cv)
        dl, dg = abs(l2 - loss) / abs(loss), np.abs(g2 - grad).max() / np.abs(grad).max()
        print(name, what, "loss moves", dl, "gradient moves", dg)
        assert dl >= 100 * LOSS_RTOL or dg >= 100 * GRAD_AREL, (what, dl, dg)


# ---------------------------------------------------------------------------------------------
# the pullback of the VJP launch (csrc/transport.hip), restated in numpy
# ---------------------------------------------------------------------------------------------
def transport_vjp_np(u, lam, nu, masks, vals, f, adv, kappa, tau, react, J, hx, hy, ngp, first, *, scale=False, dtype=np.float64, tables=None):
    """d/du <lam, R>: the cotangent (zeroed on the Dirichlet rows of R) evaluated like a field, the hand-derived pointwise coefficients
    A' = L r'(u), B' = ax q + kx nu L_x, C' = ay q + ky nu L_y with q = L + tau (ax L_x + ay L_y), pulled back through N, Nx, Ny and
    zeroed on the Dirichlet nodes of u.  Neither the forcing nor `first` enters.  scale, dtype, tables: as in transport_torch."""
    dt = np.dtype(dtype).type
    c = lambda x: np.asarray(x, dtype=dt)                                  # noqa: E731
    w = c((q1_tables(ngp) if tables is None else tables)[2])
    u, lam, vals = c(u), c(lam), [c(x) for x in vals]
    adv, kappa, react, tau, J = [dt(x) for x in adv], [dt(x) for x in kappa], [dt(x) for x in react], dt(tau), dt(J)
    ny, nx = u.shape
    fixed = np.zeros((ny, nx), dtype=bool)
    ut = u.copy()
    for k in (0, 1):
        if masks[k] is not None:
            ut = np.where(masks[k], vals[k], ut)
            fixed |= masks[k]
    lam = np.where(fixed, dt(0), lam)
    nut = np.ones((ny, nx), dtype=dt) if nu is None else c(nu)
    out = np.zeros((ny, nx), dtype=dt)
    S = np.zeros((ny, nx), dtype=dt)
    for jg in range(ngp):
        for ig in range(ngp):
            wg = J * w[ig] * w[jg]
            Na, Nxa, Nya = _tables(ngp, hx, hy, ig, jg, tables, dt)

            def at(t, tab):
                return sum(tab[ly, lx] * t[ly:ny - 1 + ly, lx:nx - 1 + lx] for ly in (0, 1) for lx in (0, 1))

            ug, nug = at(ut, Na), at(nut, Na)
            L, Lx, Ly = at(lam, Na), at(lam, Nxa), at(lam, Nya)
            q = L + tau * (adv[0] * Lx + adv[1] * Ly)
            A = L * (react[1] + 2 * react[2] * ug + 3 * react[3] * ug ** 2)
            B = adv[0] * q + kappa[0] * nug * Lx
            Cc = adv[1] * q + kappa[1] * nug * Ly
            for (ly, lx), n_ in Na.items():
                t = wg * (n_ * A + Nxa[ly, lx] * B + Nya[ly, lx] * Cc)
                out[ly:ny - 1 + ly, lx:nx - 1 + lx] += t
                S[ly:ny - 1 + ly, lx:nx - 1 + lx] += np.abs(t)
    out = np.where(fixed, dt(0), out)
    assert out.dtype == dt, out.dtype                                          # numpy promotes silently
    return (out, np.where(fixed, dt(0), S)) if scale else out


@pytest.mark.parametrize("react", [(0.0, 0.0, 0.0, 0.0), (-0.7, 8.0, -24.0, 16.0)])
@pytest.mark.parametrize("with_nu", [False, True])
@pytest.mark.parametrize("ngp,ny,nx", [(2, 6, 7), (3, 5, 6), (4, 4, 5)])
def test_transport_hand_pullback_equals_autograd_of_the_restatement(ngp, ny, nx, with_nu, react):
    rs = np.random.default_rng(11 + ngp)
    u, lam = 2 * rs.random((ny, nx)) - 1, 2 * rs.random((ny, nx)) - 1
    m1, m2 = rs.random((ny, nx)) < 0.3, rs.random((ny, nx)) < 0.3
    m2[0, 0] = m1[0, 0] = m1[1, 2] = m2[1, 2] = True                       # overlapping conditions
    for masks, vals, first in (([m1, m2], [2 * rs.random((ny, nx)) - 1, 0.25], True), ([m1, m2], [0.3, 2 * rs.random((ny, nx)) - 1], False),
                               ([None, m2], [0.0, -0.4], False), ([None, None], [0.0, 0.0], False)):
        c = dict(nu=0.5 + rs.random((ny, nx)) if with_nu else None, masks=masks, vals=vals, f=rs.random((ngp * ngp, ny - 1, nx - 1)) - 0.5,
                 adv=(0.8, -0.6), kappa=(0.05, 0.02), tau=0.04, react=react, J=0.02, hx=0.2, hy=0.25, ngp=ngp, first=first)
        ut = torch.tensor(u, requires_grad=True)
        R = transport_torch(ut, **c)
        ref, = torch.autograd.grad((R * torch.tensor(lam)).sum(), ut)
        got = transport_vjp_np(u, lam, **c)
        scale = float(ref.abs().max())
        assert scale > 1e-3
        np.testing.assert_allclose(got, ref.numpy(), rtol=0, atol=1e-12 * scale)
