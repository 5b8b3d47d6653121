"""CPU checks of the coefficient / forcing gradient of the Poisson losses (dn_poisson_coef_grad, csrc/poisson_coef_grad.hip): the C ABI
and its ctypes binding agree and the library validates its arguments before any launch; a float64 torch restatement of the kernel's
per-point formulas, kept here, equals autograd through the float64 oracle (energy and residual, nu and f, 2-D and 3-D, rules of 2 to 4
points, two conditions with value fields, non-square meshes) to 1e-12; it reproduces the reference's topology-optimisation fixtures
(tests/golden/loss_topopt_*.npz, written by tools/gen_golden_topopt.py); and the second-order identities the host layer's double backward
is built on hold against autograd's double backward."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.fem_oracle import Oracle
from test_stokes_host import header_struct, stokes_mesh

# DESIGN.md section 2, fp32 references: scalar losses rtol 1e-5, gradients rtol 1e-4 / atol 1e-4 max|ref|
LOSS_RTOL, GRAD_RTOL, GRAD_AREL = 1e-5, 1e-4, 1e-4


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_coef_grad_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    assert hasattr(h, "dn_poisson_coef_grad") and "dn_poisson_coef_grad" in _lib.SYMBOLS
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    got = [(n, getattr(t, "_length_", 1)) for n, t in _lib.DnCoefGradArgs._fields_]
    assert got == header_struct("dn_coef_grad_args")
    assert [n for n, _ in got] == ["u", "v", "bc", "a_nu", "a_f", "wscale", "in_scale", "g_nu", "g_f"]
    assert C.sizeof(_lib.DnCoefGradArgs) == 16 + 2 * C.sizeof(_lib.DnDirichlet) + 16 + 24        # the C layout (x86-64)


def test_coef_grad_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    h = _lib.lib()
    fn = h.dn_poisson_coef_grad
    m = stokes_mesh()
    assert fn(None, None, None) == -1 and fn(C.byref(m), None, None) == -1
    a = _lib.DnCoefGradArgs()
    assert fn(C.byref(m), C.byref(a), None) == -1          # no field
    a.u = 16
    assert fn(C.byref(m), C.byref(a), None) == -1          # a field but no output: rejected before anything touches the pointers
    a.g_f = 64
    a.bc[1].field = 128                                    # a value field without its mask
    assert fn(C.byref(m), C.byref(a), None) == -1
    a.bc[1].field = None
    for kind in (_lib.MASK_BITS, _lib.MASK_BOX):           # compact masks are expanded by the caller
        a.bc[0].mask_kind = kind
        assert fn(C.byref(m), C.byref(a), None) == -2
    a.bc[0].mask_kind = 7
    assert fn(C.byref(m), C.byref(a), None) == -1
    a.bc[0].mask_kind = _lib.MASK_F32
    a.bc[0].mask, a.bc[1].mask, a.bc[1].mask_kind = 256, 512, _lib.MASK_U8        # two images of different formats
    assert fn(C.byref(m), C.byref(a), None) == -2
    a.bc[1].mask_kind = _lib.MASK_F32
    a.bc[0].mask_batched = 2
    assert fn(C.byref(m), C.byref(a), None) == -1
    a.bc[0].mask_batched = 0
    for field, bad, rc in (("degree", 2, -2), ("degree", 3, -2), ("ngp", 5, -2), ("ngp", 1, -2), ("nsd", 1, -2), ("nx", 1, -1), ("batch", 0, -1)):
        mm = stokes_mesh()
        setattr(mm, field, bad)
        assert fn(C.byref(mm), C.byref(a), None) == rc, field
    gx, gw = gauss_rule(3)
    m3 = FemGeometry(3, (5, 5, 5), (0.25,) * 3, 2, 3, gx, gw).mesh_struct(1)      # 3-D Q2
    assert fn(C.byref(m3), C.byref(a), None) == -2


def test_coef_grad_ops_refuse_cpu_tensors_and_unsupported_meshes():
    from diffnet_amd import DiffNet2DFEM, ops
    from diffnet_amd._lib import DiffNetHipError
    m = DiffNet2DFEM(None, domain_size=9)
    u = torch.zeros((1, 1, 9, 9))
    with pytest.raises(DiffNetHipError):
        ops.poisson_coef_grad(m.geom, u)
    with pytest.raises(DiffNetHipError):
        m.energy_loss_and_grads(u)
    with pytest.raises(ValueError):
        ops.energy_loss_and_grads(m.geom, u, wrt=("rho",))
    assert ops.energy_loss_and_grads is not None and hasattr(m, "energy_loss_and_grads")


def test_coef_grad_switch_is_a_host_switch():
    """COEF_GRAD is stored by dn_config_set and mirrored like the kernel switches; "composed" turns the fused route off."""
    from diffnet_amd import DiffNet2DFEM, _lib, ops
    m = DiffNet2DFEM(None, domain_size=9)
    u = torch.zeros((1, 1, 9, 9))
    try:
        _lib.config_set("COEF_GRAD", "composed")
        assert _lib.config_get("COEF_GRAD") == "composed" and _lib.CONFIG_MIRROR["COEF_GRAD"] == "composed"
        assert not ops._coef_route(m.geom, u, None, ())
    finally:
        _lib.config_set("COEF_GRAD", "")
    assert _lib.config_get("COEF_GRAD") == ""
    assert not ops._coef_route(m.geom, u, None, ())           # a CPU tensor never takes the fused route
    m2 = DiffNet2DFEM(None, domain_size=9, fem_basis_deg=2)
    assert m2.geom.deg == 2


# ---------------------------------------------------------------------------------------------
# float64 restatement of the kernel's per-point formulas
# ---------------------------------------------------------------------------------------------
def oracle64(**kw):
    o = Oracle(**kw)
    o.t = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in o.t.items()}
    o.gpw = o.gpw.double()
    return o


def _corner(x, idx):
    """x[..., idx_d : n_d - 1 + idx_d]: the nodes that are local node `idx` of their element."""
    sl = [slice(None), 0] + [slice(i, x.shape[2 + d] - 1 + i) for d, i in enumerate(idx)]
    return x[tuple(sl)]


def restate(o, u, v, dirichlet, a_nu, a_f, wscale, *, scale=False, dtype=None):
    """(g_nu, g_f) as csrc/poisson_coef_grad.hip forms them, Gauss point by Gauss point, from the oracle's own tables:
        g_nu[a] = a_nu sum_e sum_g W_g N_a(g) grad v_g . grad u~_g,   g_f[a] = a_f sum_e sum_g W_g N_a(g) v_g
    u~: u after the conditions, in order; v: zero on every Dirichlet node (None: v = u~).
    dtype: the same statements in that type, with the oracle's tables, the constants and the inputs cast once at entry (None: as they
    come); scale: also returns (S_nu, S_f), the sum of |placed term| over the terms that make up each node's value."""
    nsd = o.nsd
    dtype = u.dtype if dtype is None else dtype
    u = u.to(dtype)
    v = None if v is None else v.to(dtype)
    dirichlet = [(mask, val.to(dtype) if isinstance(val, torch.Tensor) else val) for mask, val in dirichlet]
    ut, free = u, torch.ones_like(u, dtype=torch.bool)
    for mask, val in dirichlet:
        fixed = mask > 0.5
        ut = torch.where(fixed, val + u * 0.0, ut)
        free = free & ~fixed
    vv = ut if v is None else torch.where(free, v, torch.zeros_like(v))
    N = o.t["N_gp"].to(dtype)
    dN = [o.t[n].to(dtype) for n in ("dN_x_gp", "dN_y_gp", "dN_z_gp")[:nsd]]
    W = o.gpw.to(dtype) * wscale
    locs = list(itertools.product((0, 1), repeat=nsd))
    g_nu, g_f = torch.zeros_like(u), torch.zeros_like(u)
    s_nu, s_f = torch.zeros_like(u), torch.zeros_like(u)
    for g in range(N.shape[0]):
        vg = sum(N[g, 0, 0][i] * _corner(vv, i) for i in locs)
        dot = sum(sum(t[g, 0, 0][i] * _corner(vv, i) for i in locs) * sum(t[g, 0, 0][i] * _corner(ut, i) for i in locs) for t in dN)
        for i in locs:
            sl = (slice(None), 0) + tuple(slice(k, u.shape[2 + d] - 1 + k) for d, k in enumerate(i))
            t_nu, t_f = a_nu * W[g] * N[g, 0, 0][i] * dot, a_f * W[g] * N[g, 0, 0][i] * vg
            g_nu[sl] = g_nu[sl] + t_nu
            g_f[sl] = g_f[sl] + t_f
            if scale:
                s_nu[sl] = s_nu[sl] + t_nu.abs()
                s_f[sl] = s_f[sl] + t_f.abs()
    assert g_nu.dtype == dtype and g_f.dtype == dtype, (g_nu.dtype, g_f.dtype)
    return (g_nu, g_f, s_nu, s_f) if scale else (g_nu, g_f)


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)


def _case(nsd, sizes, ngp, B, seed, nbc=2, fields=True):
    """Oracle + seeded fields on a mesh of `sizes` nodes (x, y[, z]); conditions: two random blobs, the second with a value field."""
    o = oracle64(nsd=nsd, domain_sizes=tuple(sizes) + (1,) * (3 - nsd), domain_lengths=(1.0, 0.7, 1.3), ngp_1d=ngp)
    shape = (B, 1, *tuple(sizes)[::-1])
    u, nu, f, lam = _rand(shape, seed), _rand(shape, seed + 1, 0.5, 1.5), _rand(shape, seed + 2), _rand(shape, seed + 3)
    dl = []
    for k in range(nbc):
        mask = (_rand(shape, seed + 10 + k, 0.0, 1.0) < 0.2).double()
        val = _rand(shape, seed + 20 + k) if (fields and k == 1) else torch.tensor(0.3 - 0.5 * k, dtype=torch.float64)
        dl.append((mask, val))
    return o, u, nu, f, lam, dl


CASES = [(2, (9, 7), 2, 2), (2, (6, 11), 3, 1), (2, (8, 5), 4, 2), (3, (5, 4, 6), 2, 2), (3, (4, 5, 3), 3, 1), (3, (3, 4, 5), 4, 1)]


def _close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


@pytest.mark.parametrize("nsd,sizes,ngp,B", CASES)
def test_restatement_equals_autograd_of_the_oracle_energy(nsd, sizes, ngp, B):
    o, u, nu, f, _, dl = _case(nsd, sizes, ngp, B, 100 + ngp)
    c, jac = 0.5, 0.37
    nu.requires_grad_(True)
    f.requires_grad_(True)
    L = o.energy(u, nu=nu, f=f, dirichlet=dl, c=c, jac=jac)
    rn, rf = torch.autograd.grad(L, (nu, f))
    s = 1.0 / (B * int(np.prod(o.spec.nel)))
    g_nu, g_f = restate(o, u, None, dl, s * c, -s, jac)
    _close(g_nu, rn)
    _close(g_f, rf)


@pytest.mark.parametrize("nsd,sizes,ngp,B", CASES)
def test_restatement_equals_autograd_of_the_oracle_residual(nsd, sizes, ngp, B):
    o, u, nu, f, lam, dl = _case(nsd, sizes, ngp, B, 200 + ngp)
    jac = 1.7
    nu.requires_grad_(True)
    f.requires_grad_(True)
    R = o.residual(u, nu=nu, f=f, dirichlet=dl, jac=jac, zero_masks=[m for m, _ in dl])
    rn, rf = torch.autograd.grad((lam * R).sum(), (nu, f))
    g_nu, g_f = restate(o, u, lam, dl, 1.0, -1.0, jac)
    _close(g_nu, rn)
    _close(g_f, rf)
    # residual_loss: lambda = 2 R
    rn2, rf2 = torch.autograd.grad((o.residual(u, nu=nu, f=f, dirichlet=dl, jac=jac, zero_masks=[m for m, _ in dl]) ** 2).sum(), (nu, f))
    g_nu, g_f = restate(o, u, 2.0 * R.detach(), dl, 1.0, -1.0, jac)
    _close(g_nu, rn2)
    _close(g_f, rf2)


@pytest.mark.parametrize("nsd,sizes,ngp,B", CASES)
def test_transpose_identity_on_random_fields(nsd, sizes, ngp, B):
    """<mu, g_nu(u~)> = <u~, K_mu u~>: the coefficient gradient is the transpose of the stiffness operator in its coefficient."""
    o, u, _, _, mu, _ = _case(nsd, sizes, ngp, B, 300 + ngp, nbc=0)
    g_nu, _ = restate(o, u, None, [], 1.0, 1.0, 0.9)
    Ku = o.residual(u, nu=mu, jac=0.9)
    np.testing.assert_allclose(float((mu * g_nu).sum()), float((u * Ku).sum()), rtol=1e-12)


@pytest.mark.parametrize("nsd,sizes,ngp,B", CASES[:2] + CASES[3:4])
def test_second_order_identities_equal_autograd_double_backward(nsd, sizes, ngp, B):
    o, u, _, _, lam, dl = _case(nsd, sizes, ngp, B, 400 + ngp)
    mu, mu_f = _rand(u.shape, 7), _rand(u.shape, 8)
    a_nu, a_f, jac = 0.8, -1.3, 0.6
    masks = [m for m, _ in dl]
    zero = torch.zeros_like(u)
    hom = [(m, torch.tensor(0.0, dtype=torch.float64)) for m in masks]
    # v given: the pullbacks to v and to u
    ur, vr = u.clone().requires_grad_(True), lam.clone().requires_grad_(True)
    g_nu, g_f = restate(o, ur, vr, dl, a_nu, a_f, jac)
    du, dv = torch.autograd.grad((mu * g_nu).sum() + (mu_f * g_f).sum(), (ur, vr))
    want_v = a_nu * o.residual(u, nu=mu, dirichlet=dl, jac=jac, zero_masks=masks) - a_f * o.residual(zero, f=mu_f, jac=jac, zero_masks=masks)
    want_u = a_nu * o.residual(lam, nu=mu, dirichlet=hom, jac=jac, zero_masks=masks)
    _close(dv, want_v)
    _close(du, want_u)
    # v absent: one launch of the energy-gradient operator with (nu, f) := (a_nu mu, -a_f mu_f), alpha = 2, beta = 1
    ur = u.clone().requires_grad_(True)
    g_nu, g_f = restate(o, ur, None, dl, a_nu, a_f, jac)
    du, = torch.autograd.grad((mu * g_nu).sum() + (mu_f * g_f).sum(), ur)
    want = 2.0 * o.residual(u, nu=a_nu * mu, dirichlet=dl, jac=jac, zero_masks=masks) + o.residual(zero, f=-a_f * mu_f, jac=jac, zero_masks=masks)
    _close(du, want)


# ---------------------------------------------------------------------------------------------
# the reference's topology-optimisation losses
# ---------------------------------------------------------------------------------------------
def topopt_fixture(name):
    z = np.load(os.path.join(GOLDEN, name))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", ["loss_topopt_n17.npz", "loss_topopt_n33.npz"])
def test_restatement_reproduces_the_reference_topopt_losses(name):
    z = topopt_fixture(name)
    n = z["u"].shape[-1]
    o = oracle64(nsd=2, domain_size=n)
    u, rho, f = (torch.from_numpy(z[k]).double() for k in ("u", "rho", "f"))
    bc1, bc2 = (torch.from_numpy(z["inputs"][:, k:k + 1]).double() for k in (0, 1))
    sg = torch.sigmoid(rho)
    nu = 0.001 + sg ** 3
    s = 1.0 / (n - 1) ** 2
    # loss = 0.5 nu grad u . grad u - u f (no substitution) + the penalties
    ur = u.clone().requires_grad_(True)
    L = o.energy(ur, nu=nu, f=f, c=0.5)
    gu, = torch.autograd.grad(L, ur)
    np.testing.assert_allclose(float(L), float(z["loss"]) - float(z["dbc"]), rtol=LOSS_RTOL)
    ref_u = z["loss_du"] - z["dbc_du"]
    np.testing.assert_allclose(gu.numpy(), ref_u, rtol=GRAD_RTOL, atol=GRAD_AREL * np.abs(ref_u).max())
    g_nu, _ = restate(o, u, None, [], s * 0.5, -s, 1.0)
    g_rho = g_nu * 3.0 * sg ** 3 * (1.0 - sg)
    np.testing.assert_allclose(g_rho.numpy(), z["loss_drho"], rtol=GRAD_RTOL, atol=GRAD_AREL * np.abs(z["loss_drho"]).max())
    assert np.abs(z["loss_drho"]).max() > 0.1
    # compliance = -u~ f with both conditions applied: the c = 0 form
    one, nil = torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)
    dl = [(bc1, one), (bc2, nil)]
    ur = u.clone().requires_grad_(True)
    Cv = o.energy(ur, f=f, dirichlet=dl, c=0.0)
    gu, = torch.autograd.grad(Cv, ur)
    np.testing.assert_allclose(float(Cv), float(z["compliance"]), rtol=LOSS_RTOL, atol=1e-7)
    np.testing.assert_allclose(gu.numpy(), z["compliance_du"], rtol=GRAD_RTOL, atol=GRAD_AREL * np.abs(z["compliance_du"]).max())
    assert not z["compliance_drho"].any()
    # ... whose forcing gradient is g_f alone
    fr = f.clone().requires_grad_(True)
    gf_ref, = torch.autograd.grad(o.energy(u, f=fr, dirichlet=dl, c=0.0), fr)
    _, g_f = restate(o, u, None, dl, 0.0, -s, 1.0)
    _close(g_f, gf_ref)
