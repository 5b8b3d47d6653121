"""CPU checks of the fused 3-D eikonal weak-form residual (dn_eikonal3d_apply, csrc/eikonal3d.hip): the C ABI and its ctypes binding agree,
the workspace size is the header's closed formula of the launch plan and the library validates its arguments before any launch; the
reference fixtures (tests/golden/loss_eikonal3d_*.npz, written by tools/gen_golden_eikonal3d.py from the reference script's own loss
body) agree with a float64 torch restatement of the operator kept here (the script's spelling, differentiated by autograd), every one of
its terms is visible in the fixtures' residual norm, and the hand-derived pullback of the kernel's VJP mode (include/diffnet_hip.h,
DESIGN.md section 3.2), restated in numpy, equals the restatement's autograd VJP."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_transport_host import GRAD_AREL, GRAD_RTOL, LOSS_RTOL

FIXTURES = ["loss_eikonal3d_sphere_n9.npz", "loss_eikonal3d_sphere_n7_g3.npz"]


def ek3_mesh(nodes=(7, 6, 5), ngp=2, B=2, deg=1):
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    gx, gw = gauss_rule(ngp)
    return FemGeometry(3, nodes, tuple(1 / (n - 1) for n in nodes), deg, ngp, gx, gw).mesh_struct(B)


def _tiles(n, T):
    return 1 if n <= T else -(-(n - 1) // (T - 1))


def default_plan(m):
    """include/diffnet_hip.h, dn_eikonal3d_apply: (TX, TY, R) of the library's own launch plan"""
    nelz = m.nz - 1
    best, TY = -1.0, 16
    for ty in (4, 8, 12, 16):
        util = m.ny / (_tiles(m.ny, ty) * ty) + 0.002 * ty
        if util > best:
            best, TY = util, ty
    R = 32
    per_strip = _tiles(m.nx, 16) * _tiles(m.ny, TY) * m.batch
    while R > 4 and per_strip * -(-nelz // R) < 1024:
        R //= 2
    return 16, TY, max(1, min(R, nelz))


def workspace_formula(m, plan=None):
    """4160 + 8 * chunks * tiles * strips * B"""
    TX, TY, R = default_plan(m) if plan is None else plan
    return 4160 + 8 * _tiles(m.nx, TX) * _tiles(m.ny, TY) * -(-(m.nz - 1) // R) * m.batch


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_eikonal3d_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "..", "include", "diffnet_hip.h")).read()
    for s in ("dn_eikonal3d_workspace_bytes", "dn_eikonal3d_apply"):
        assert hasattr(h, s) and s in _lib.SYMBOLS and s + "(const dn_mesh *mesh" in header, s
    assert _lib.SYMBOLS["dn_eikonal3d_apply"] == _lib.SYMBOLS["dn_eikonal_apply"]          # the same argument struct
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    assert "#define DN_ABI_VERSION 10" in header
    for s in ("eikonal3d.hip", "eikonal3d_g3.hip", "eikonal3d_g4.hip"):
        assert s in build.SOURCES


def test_eikonal3d_workspace_bytes_is_the_documented_formula():
    from diffnet_amd import _lib
    h = _lib.lib()
    for ngp in (2, 3, 4):
        for nodes, B in (((2, 2, 2), 1), ((7, 6, 5), 2), ((17, 18, 4), 1), ((16, 17, 40), 3)):
            m = ek3_mesh(nodes, ngp, B)
            got = h.dn_eikonal3d_workspace_bytes(C.byref(m))
            assert got > 0 and got == workspace_formula(m), (ngp, nodes, B)
    # (65, 9, 33) at B = 3: 5 chunks x 1 tile of 12 rows, 32 planes in strips of 4;  129^3 at B = 2: 9 x 9 tiles of 16 x 16, strips of 16
    m = ek3_mesh((65, 9, 33), 2, 3)
    assert default_plan(m) == (16, 12, 4) and workspace_formula(m) == 4160 + 8 * 5 * 1 * 8 * 3
    assert h.dn_eikonal3d_workspace_bytes(C.byref(m)) == workspace_formula(m)
    m = ek3_mesh((129, 129, 129), 3, 2)
    assert default_plan(m) == (16, 16, 16) and workspace_formula(m) == 4160 + 8 * 9 * 9 * 8 * 2
    assert h.dn_eikonal3d_workspace_bytes(C.byref(m)) == workspace_formula(m)
    # "PLAN3D" "TX,TY,E,R" (E ignored) overrides the plan and with it the size; a block that is no whole number of waves is ignored
    m = ek3_mesh((41, 22, 12), 2, 3)
    try:
        for val, plan in (("8,8,1,4", (8, 8, 4)), ("16,8,2,2", (16, 8, 2)), ("16,16,1,64", (16, 16, 11)), ("32,4,1,3", (32, 4, 3)), ("8,4,1,4", None),
                          ("16,32,1,4", None), ("16,16,1,0", None)):
            assert h.dn_config_set(b"PLAN3D", val.encode()) == 0
            assert h.dn_eikonal3d_workspace_bytes(C.byref(m)) == workspace_formula(m, plan), val
    finally:
        h.dn_config_set(b"PLAN3D", b"")
    for field, bad in (("nsd", 2), ("nx", 1), ("ny", 0), ("nz", 1), ("batch", 0), ("ngp", 5), ("ngp", 1), ("degree", 2)):
        m = ek3_mesh()
        setattr(m, field, bad)
        assert h.dn_eikonal3d_workspace_bytes(C.byref(m)) == -1, field
    # the 2-D entry points keep refusing 3-D meshes
    m = ek3_mesh()
    assert h.dn_eikonal_workspace_bytes(C.byref(m)) == -1


def test_eikonal3d_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    m = ek3_mesh()
    # every pointer below is a small odd number: a check that came after a launch or a dereference would not return
    assert h.dn_eikonal3d_apply(C.byref(m), None, None) == -1
    assert h.dn_eikonal3d_apply(None, None, None) == -1
    a = _lib.DnEikonalArgs()                        # a NULL u
    a.out = 65
    assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -1
    a.out = None
    a.u = 17                                        # a field but no output at all
    assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -1
    for name in ("sumsq", "norm"):
        setattr(a, name, 129)                       # a sum without a workspace
        assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -3, name
        a.workspace, a.workspace_bytes = 257, 64    # ... or with one that is too small
        assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -3, name
        a.workspace_bytes = h.dn_eikonal3d_workspace_bytes(C.byref(m)) - 1
        assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -3, name
        setattr(a, name, None)
        a.workspace, a.workspace_bytes = None, 0
    a.out = 65
    for deg, ngp in ((2, 3), (3, 4), (0, 2), (1, 5), (1, 1)):          # a degree / ngp combination outside the domain
        mm = ek3_mesh()
        mm.degree, mm.ngp = deg, ngp
        assert h.dn_eikonal3d_apply(C.byref(mm), C.byref(a), None) == -2, (deg, ngp)
    mm = ek3_mesh()
    mm.nsd = 2
    assert h.dn_eikonal3d_apply(C.byref(mm), C.byref(a), None) == -1
    mm = ek3_mesh()
    mm.nz = 1
    assert h.dn_eikonal3d_apply(C.byref(mm), C.byref(a), None) == -1
    # packed and box masks
    for k in (0, 1):
        for kind in (_lib.MASK_BITS, _lib.MASK_BOX):
            a.bc[k].mask_kind = kind
            assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -2, (k, kind)
            a.bc[k].mask, a.bc[k].box_faces = 513, 15
            assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -2, (k, kind)
            a.bc[k].mask, a.bc[k].box_faces = None, 0
        a.bc[k].mask_kind = 7                       # an unknown mask kind
        assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -1
        a.bc[k].mask_kind = 0
        a.bc[k].field = 121                         # a value field without its mask
        assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -1
        a.bc[k].field = None
        for flag in ("mask_batched", "field_batched"):
            setattr(a.bc[k], flag, 2)
            assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -1, flag
            setattr(a.bc[k], flag, 0)
    for flag, bad in (("f_batched", 2), ("vjp", 2), ("vjp", -1)):
        setattr(a, flag, bad)
        assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -1, flag
        setattr(a, flag, 0)
    a.f, a.f_gp = 33, 49                            # nodal and Gauss-point forcing at once
    assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -1
    a.f, a.f_gp = None, None
    a.vjp = 1                                       # a VJP without its cotangent
    assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -1
    a.cot = 81
    a.in_den = 97                                   # in_den without in_num
    assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -1
    a.vjp, a.cot, a.in_den = 0, None, None
    a.in_num = 97                                   # in_num outside the VJP
    assert h.dn_eikonal3d_apply(C.byref(m), C.byref(a), None) == -1


def test_eikonal3d_ops_refuse_cpu_tensors_and_bad_arguments():
    from diffnet_amd import DiffNet2DFEM, DiffNet3DFEM, ops
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd import eikonal as ek
    m = DiffNet3DFEM(None, domain_size=5, nsd=3)
    u = torch.zeros((1, 1, 5, 5, 5))
    with pytest.raises(DiffNetHipError):
        ops.eikonal3d_apply(m.geom, u)               # a CPU tensor
    for fn in (ek.eikonal_residual, ek.eikonal_loss, ek.eikonal_loss_and_grad):
        with pytest.raises(DiffNetHipError):
            fn(m, u, tau=0.25)
    for fn in (ek.eikonal_loss, ek.eikonal_loss_and_grad):
        with pytest.raises(ValueError):
            fn(m, u, kind="max")
    with pytest.raises(ValueError):
        ops.eikonal3d_apply(m.geom, u, bc_values=(0.0,))
    with pytest.raises(ValueError):
        ops.eikonal3d_apply(m.geom, u, want_out=False)
    with pytest.raises(ValueError):
        ops.eikonal3d_apply(m.geom, u, in_num=torch.ones(1))          # a scale without a cotangent
    with pytest.raises(ValueError):
        ops.eikonal3d_apply(m.geom, u, cot=u, in_den=torch.ones(1))   # in_den without in_num
    # a 2-D geometry is not this operator's, a 3-D one not the 2-D operator's
    m2 = DiffNet2DFEM(None, domain_size=5)
    with pytest.raises(DiffNetHipError, match="3-D"):
        ops.eikonal3d_apply(m2.geom, torch.zeros((1, 1, 5, 5)))
    with pytest.raises(DiffNetHipError):
        ops.eikonal_apply(m.geom, u)
    # a 3-D Q2 mesh: the fused functions name the composed route
    mq = DiffNet3DFEM(None, domain_size=5, nsd=3, fem_basis_deg=2)
    for fn in (ek.eikonal_residual, ek.eikonal_loss, ek.eikonal_loss_and_grad):
        with pytest.raises(DiffNetHipError, match="eikonal_residual_composed"):
            fn(mq, u, tau=0.25)
    with pytest.raises(DiffNetHipError, match="eikonal_residual_composed"):
        ops.eikonal3d_apply(mq.geom, u)
    # the default wscale of a 3-D mesh
    assert ek._coef(m, 0.25, None, None) == dict(tau=0.25, sq=1.25, wscale=(0.5 * m.hx) * (0.5 * m.hy) * (0.5 * m.hz))


# ---------------------------------------------------------------------------------------------
# float64 restatement of the operator, in the script's spelling (torch, differentiable) and the pullback by hand (numpy)
# ---------------------------------------------------------------------------------------------
def _tables(ngp, hx, hy, hz):
    from diffnet_amd.tables import Basis1D, gauss_rule
    gx, gw = gauss_rule(ngp)
    Bt, Dt = Basis1D(1).at_gauss(gx)[:2]            # (ngp, 2)
    return np.asarray(Bt, dtype=np.float64), np.asarray(Dt, dtype=np.float64), np.asarray(gw, dtype=np.float64), 2.0 / hx, 2.0 / hy, 2.0 / hz


def _loc(nel, kb, jb, ib):
    nelz, nely, nelx = nel
    return (slice(kb, kb + nelz), slice(jb, jb + nely), slice(ib, ib + nelx))


def _gauss_points(ngp, hx, hy, hz, wscale):
    """(g, W, N, Nx, Ny, Nz) per Gauss point, g = (kg * ngp + jg) * ngp + ig as gauss_pt_evaluation orders them; the tables map a local
    node (kb, jb, ib) to its basis value"""
    Bt, Dt, gw, sx, sy, sz = _tables(ngp, hx, hy, hz)
    nodes = [(kb, jb, ib) for kb in (0, 1) for jb in (0, 1) for ib in (0, 1)]
    for kg in range(ngp):
        for jg in range(ngp):
            for ig in range(ngp):
                W = wscale * gw[ig] * gw[jg] * gw[kg]
                N = {a: Bt[ig, a[2]] * Bt[jg, a[1]] * Bt[kg, a[0]] for a in nodes}
                Nx = {a: Dt[ig, a[2]] * sx * Bt[jg, a[1]] * Bt[kg, a[0]] for a in nodes}
                Ny = {a: Bt[ig, a[2]] * Dt[jg, a[1]] * sy * Bt[kg, a[0]] for a in nodes}
                Nz = {a: Bt[ig, a[2]] * Bt[jg, a[1]] * Dt[kg, a[0]] * sz for a in nodes}
                yield (kg * ngp + jg) * ngp + ig, W, N, Nx, Ny, Nz


def eikonal3d_t64(u, hx, hy, hz, ngp, tau, sq=None, f=1.0, wscale=None, masks=(None, None), vals=(0.0, 0.0), drop=None):
    """R (nz, ny, nx) of the header's formula from u (nz, ny, nx), a float64 torch tensor (differentiable): the script's sum over the Gauss
    points of JxW (tau u (dN_x u_x + dN_y u_y + dN_z u_z) + sq N (u_x^2 + u_y^2 + u_z^2) - N f), assembled, zero on the Dirichlet nodes.
    f: a float, a nodal (nz, ny, nx) tensor or a Gauss-point (G, nelz, nely, nelx) one.  drop: "stab" | "sq" | "rhs" leaves that term out,
    "dz" every z-derivative."""
    sq = 1.0 + tau if sq is None else sq
    wscale = (0.5 * hx) * (0.5 * hy) * (0.5 * hz) if wscale is None else wscale
    nel = tuple(n - 1 for n in u.shape)
    ut = u
    fixed = torch.zeros(u.shape, dtype=torch.bool)
    for k in (0, 1):
        if masks[k] is not None:
            mk = torch.as_tensor(masks[k], dtype=torch.bool)
            v = vals[k] if isinstance(vals[k], torch.Tensor) else torch.full_like(u, float(vals[k]))
            ut = torch.where(mk, v, ut)
            fixed |= mk
    out = torch.zeros(u.shape, dtype=torch.float64)
    zs = 0.0 if drop == "dz" else 1.0
    for g, W, N, Nx, Ny, Nz in _gauss_points(ngp, hx, hy, hz, wscale):
        def at(t, tab):
            return sum(tab[a] * t[_loc(nel, *a)] for a in tab)

        ug, ux, uy, uz = at(ut, N), at(ut, Nx), at(ut, Ny), zs * at(ut, Nz)
        if isinstance(f, torch.Tensor) and f.dim() == 4:
            fg = f[g]
        elif isinstance(f, torch.Tensor):
            fg = at(f, N)
        else:
            fg = torch.full_like(ug, float(f))
        for a in N:
            t = 0.0
            if drop != "stab":
                t = t + tau * ug * (Nx[a] * ux + Ny[a] * uy + zs * Nz[a] * uz)
            if drop != "sq":
                t = t + sq * N[a] * (ux ** 2 + uy ** 2 + uz ** 2)
            if drop != "rhs":
                t = t - N[a] * fg
            sl = _loc(nel, *a)
            out[sl] = out[sl] + W * t
    return torch.where(fixed, torch.zeros_like(out), out)


def eikonal3d_pullback_np(u, cot, hx, hy, hz, ngp, tau, sq=None, wscale=None, masks=(None, None), vals=(0.0, 0.0)):
    """The VJP of the header: with the cotangent (zero on the Dirichlet nodes) evaluated like a field (L, grad L),
    A' = tau grad L . grad u, (B', C', D') = 2 sq L grad u + tau u grad L on N | Nx | Ny | Nz, assembled, zero on the Dirichlet nodes"""
    sq = 1.0 + tau if sq is None else sq
    wscale = (0.5 * hx) * (0.5 * hy) * (0.5 * hz) if wscale is None else wscale
    nel = tuple(n - 1 for n in u.shape)
    ut, fixed = np.array(u, dtype=np.float64), np.zeros(u.shape, dtype=bool)
    for k in (0, 1):
        if masks[k] is not None:
            ut = np.where(masks[k], vals[k], ut)
            fixed |= np.asarray(masks[k], dtype=bool)
    lt = np.where(fixed, 0.0, cot)
    out = np.zeros(u.shape)
    for g, W, N, Nx, Ny, Nz in _gauss_points(ngp, hx, hy, hz, wscale):
        def at(t, tab):
            return sum(tab[a] * t[_loc(nel, *a)] for a in tab)

        ug, ux, uy, uz = at(ut, N), at(ut, Nx), at(ut, Ny), at(ut, Nz)
        L, Lx, Ly, Lz = at(lt, N), at(lt, Nx), at(lt, Ny), at(lt, Nz)
        A = tau * (Lx * ux + Ly * uy + Lz * uz)
        Bc = 2.0 * sq * L * ux + tau * ug * Lx
        Cc = 2.0 * sq * L * uy + tau * ug * Ly
        Dc = 2.0 * sq * L * uz + tau * ug * Lz
        for a in N:
            out[_loc(nel, *a)] += W * (N[a] * A + Nx[a] * Bc + Ny[a] * Cc + Nz[a] * Dc)
    return np.where(fixed, 0.0, out)


def fixture_case(z):
    kw = eval(str(z["kwargs"]))
    n = kw["domain_size"]
    h = 1.0 / (n - 1)
    return dict(hx=h, hy=h, hz=h, ngp=kw.get("ngp_1d", 2), tau=float(z["tau"]), sq=float(z["sq"]), wscale=float(z["wscale"]))


def fixture_norm_and_grad(z, drop=None):
    """(||R||_F, its gradient, R) of the restatement on the fixture's u"""
    u = torch.tensor(z["u"][0, 0].astype(np.float64), requires_grad=True)
    R = eikonal3d_t64(u, drop=drop, **fixture_case(z))
    nrm = torch.norm(R)
    g, = torch.autograd.grad(nrm, u)
    return float(nrm.detach()), g.numpy(), R.detach().numpy()


def fixture_norm64(z):
    """the float64 norm of the fixture's R1: what ||R|| is compared with (loss = ||R|| + 1 would hide a 3e-4 error of the norm)"""
    return float(np.sqrt(np.sum(z["R1"].astype(np.float64) ** 2)))


@pytest.mark.parametrize("name", FIXTURES)
def test_eikonal3d_fixtures_agree_with_float64_restatement(name):
    z = np.load(os.path.join(GOLDEN, name))
    for k in ("kwargs", "script", "u", "pc", "tau", "sq", "wscale", "R1", "point_terms", "loss", "grad"):
        assert k in z.files, (name, k)
    assert float(z["tau"]) == 0.25 and float(z["sq"]) == 1.25 and float(z["point_terms"]) == 1.0
    assert "05_3d_sphere_loss4.py" in str(z["script"]) and z["u"].ndim == 5 and z["R1"].shape == z["u"].shape[2:]
    nrm, grad, R = fixture_norm_and_grad(z)
    ref, ref_nrm = z["grad"][0, 0], fixture_norm64(z)
    print(name, "||R|| rel", abs(nrm - ref_nrm) / ref_nrm, "grad", np.abs(grad - ref).max() / np.abs(ref).max(),
          "R1", np.abs(R - z["R1"]).max() / np.abs(z["R1"]).max())
    np.testing.assert_allclose(nrm, ref_nrm, rtol=LOSS_RTOL)
    np.testing.assert_allclose(nrm + float(z["point_terms"]), float(z["loss"]), rtol=LOSS_RTOL)        # in addition: dominated by the constant
    np.testing.assert_allclose(grad, ref, rtol=GRAD_RTOL, atol=GRAD_AREL * np.abs(ref).max())
    np.testing.assert_allclose(R, z["R1"], rtol=GRAD_RTOL, atol=GRAD_AREL * np.abs(z["R1"]).max())
    # the neutral point: u is exactly 0 on the nodes around its element, and |grad u| = O(1) elsewhere
    n = z["u"].shape[-1]
    k = int(float(z["pc"][0]) * (n - 1))
    assert np.all(z["u"][0, 0, k:k + 3, k:k + 3, k:k + 3] == 0.0) and 0.1 < np.abs(z["u"]).max() < 1.0


@pytest.mark.parametrize("name", FIXTURES)
def test_eikonal3d_every_term_is_visible_in_the_fixtures(name):
    z = np.load(os.path.join(GOLDEN, name))
    ref = fixture_norm64(z)
    for drop in ("stab", "sq", "rhs", "dz"):
        nrm, _, _ = fixture_norm_and_grad(z, drop=drop)
        print(name, "without", drop, "||R|| moves by", abs(nrm - ref) / ref, "relative")
        assert abs(nrm - ref) >= 100 * LOSS_RTOL * ref, (name, drop)


@pytest.mark.parametrize("ngp", [2, 3, 4])
def test_eikonal3d_pullback_by_hand_equals_autograd_of_the_restatement(ngp):
    nx, ny, nz = 4, 3, 5
    shp = (nz, ny, nx)
    rs = np.random.default_rng(11 + ngp)
    m1, m2 = rs.random(shp) < 0.2, rs.random(shp) < 0.2
    m1[0, 0, 0] = m2[0, 0, 0] = True                # the two conditions overlap
    m1[1, 1, 1], m2[1, 1, 1] = False, False
    v1, v2 = 2 * rs.random(shp) - 1, 2 * rs.random(shp) - 1
    u0, cot = 2 * rs.random(shp) - 1, 2 * rs.random(shp) - 1
    c = dict(hx=0.2, hy=0.25, hz=0.4, ngp=ngp, tau=0.25, sq=1.4, wscale=0.8)
    for masks, vals in (((None, None), (0.0, 0.0)), ((m1, m2), (v1, v2))):
        u = torch.tensor(u0, requires_grad=True)
        R = eikonal3d_t64(u, f=torch.tensor(rs.random(shp)), masks=masks, vals=tuple(torch.as_tensor(v, dtype=torch.float64) for v in vals), **c)
        g, = torch.autograd.grad(R, u, torch.tensor(cot))
        mine = eikonal3d_pullback_np(u0, cot, masks=masks, vals=vals, **c)
        assert np.abs(g.numpy()).max() > 1e-2
        np.testing.assert_allclose(mine, g.numpy(), rtol=0, atol=1e-12 * np.abs(g.numpy()).max())
        if masks[0] is not None:
            assert np.all(mine[m1 | m2] == 0.0) and np.all(R.detach().numpy()[m1 | m2] == 0.0)
