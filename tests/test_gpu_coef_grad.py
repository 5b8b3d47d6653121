"""The coefficient / forcing gradient of the Poisson losses on the GPU (dn_poisson_coef_grad, ops.poisson_coef_grad, the autograd routing of
energy_loss / residual / residual_loss, DiffNetFEM.energy_loss_and_grads): against autograd through the composed operators on ragged
shapes, against the reference's topology-optimisation fixtures, bitwise reproducibility across runs, batch sizes and launch plans, two exact
checks, the routing and its switch, the Hessian-vector product, isolation from the chained launches of other operators, HIP-graph capture,
full-size properties and the example in both modes.  Tolerances: DESIGN.md section 2 (scalars rtol 1e-5, gradients rtol 1e-4 with
atol 1e-4 max|ref|)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_parity import boundary_mask, dev, module, seeded

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_RTOL, GRAD_AREL = 1e-5, 1e-4, 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gclose(got, ref, msg=""):
    got, ref = got.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=GRAD_RTOL, atol=GRAD_AREL * max(1e-30, float(np.abs(ref).max())), err_msg=msg)


def rect_module(nx, ny, ngp, lengths=(1.0, 0.7)):
    return module(dict(domain_sizes=(nx, ny), domain_lengths=lengths, domain_size=nx, domain_length=lengths[0], ngp_1d=ngp))


def box_module(nx, ny, nz, ngp):
    return module(dict(nsd=3, domain_sizes=(nx, ny, nz), domain_lengths=(1.0, 0.8, 1.2), domain_size=nx, domain_length=1.0, ngp_1d=ngp))


def blob(shape, seed, frac=0.15):
    return (seeded(shape, seed) < frac).float()


def conditions(shape, B, seed, nbc, kind, fields):
    """nbc conditions on random blobs: mask format `kind` (f32 / u8 / bool), the first shared by the batch, the second with a value field
    when `fields`."""
    dl = []
    for k in range(nbc):
        ms = (1 if k == 0 else B, *shape[1:])
        m = blob(ms, seed + k).to(dev())
        m = m if kind == "f32" else (m.to(torch.uint8) if kind == "u8" else m > 0.5)
        val = seeded(shape, seed + 7 + k, -0.5).to(dev()) if (fields and k == nbc - 1) else 0.3 - 0.5 * k
        dl.append((m, val))
    return dl


def reference_grads(m, u, nu, f, lam, dl, c, jac):
    """autograd through the composed operators: d energy / d(nu, f) and d <lam, R> / d(nu, f), per sample"""
    from diffnet_amd import ops
    B = u.shape[0]
    nur = (nu.expand_as(u) if nu.shape[0] != B else nu).clone().requires_grad_(True)
    fr = (f.expand_as(u) if f.shape[0] != B else f).clone().requires_grad_(True)
    E = ops.composed_energy(m.geom, u, nur, fr, None, dl, c, jac)
    en, ef = torch.autograd.grad(E, (nur, fr))
    R = ops.composed_residual(m.geom, u, nur, fr, None, dl, jac)
    rn, rf = torch.autograd.grad((lam * R).sum(), (nur, fr))
    return en, ef, rn, rf


# ---------------------------------------------------------------------------------------------
# 1. the raw launch against autograd through the composed operators
# ---------------------------------------------------------------------------------------------
SHAPES_2D = [(61, 9, 2, 1, 2, "f32", True), (62, 17, 3, 2, 1, "u8", False), (63, 8, 4, 5, 2, "bool", True), (124, 13, 2, 2, 0, "f32", False),
             (125, 33, 3, 1, 2, "u8", True), (17, 70, 2, 5, 1, "f32", True), (33, 41, 4, 2, 2, "u8", False), (129, 25, 2, 1, 1, "bool", False)]


@pytest.mark.parametrize("nx,ny,ngp,B,nbc,kind,fields", SHAPES_2D)
def test_raw_launch_matches_composed_autograd_2d(nx, ny, ngp, B, nbc, kind, fields):
    from diffnet_amd import ops
    m = rect_module(nx, ny, ngp)
    shape = (B, 1, ny, nx)
    u, lam = seeded(shape, 1, -0.5).to(dev()), seeded(shape, 2, -0.5).to(dev())
    nu = seeded((1 if B == 2 else B, 1, ny, nx), 3, 0.5).to(dev())           # shared by the batch at B = 2
    f = seeded((1 if B == 5 else B, 1, ny, nx), 4, -0.5).to(dev())
    dl = conditions(shape, B, 10, nbc, kind, fields)
    c, jac = 0.5, 0.37
    s = 1.0 / (B * m.geom.nelem_total)
    en, ef, rn, rf = reference_grads(m, u, nu, f, lam, dl, c, jac)
    g_nu, g_f = ops.poisson_coef_grad(m.geom, u, None, dl, s * c, -s, jac)
    gclose(g_nu, en, "energy d/dnu")
    gclose(g_f, ef, "energy d/df")
    g_nu, g_f = ops.poisson_coef_grad(m.geom, u, lam, dl, 1.0, -1.0, jac)
    gclose(g_nu, rn, "residual VJP d/dnu")
    gclose(g_f, rf, "residual VJP d/df")
    # one output at a time and the device scale
    sc = torch.tensor([-2.5], device=dev())
    only_nu, none = ops.poisson_coef_grad(m.geom, u, lam, dl, 1.0, -1.0, jac, want=("nu",), in_scale=sc)
    assert none is None
    gclose(only_nu, -2.5 * rn, "in_scale")
    none, only_f = ops.poisson_coef_grad(m.geom, u, lam, dl, 1.0, -1.0, jac, want="f")
    assert none is None and torch.equal(only_f, g_f)
    # shared nu / f through autograd: the sum over the samples
    nur, fr = nu.clone().requires_grad_(True), f.clone().requires_grad_(True)
    m.energy_loss(u, nur, fr, dirichlet=dl, c=c, jac=jac).backward()
    gclose(nur.grad, en.sum(0, keepdim=True) if nu.shape[0] != B else en, "autograd d/dnu")
    gclose(fr.grad, ef.sum(0, keepdim=True) if f.shape[0] != B else ef, "autograd d/df")


@pytest.mark.parametrize("sizes,ngp,B,nbc,kind,fields", [((9, 9, 9), 2, 2, 2, "f32", True), ((12, 10, 14), 3, 1, 1, "u8", False),
                                                         ((12, 10, 14), 4, 5, 2, "bool", True), ((33, 33, 33), 2, 1, 2, "u8", False)])
def test_raw_launch_matches_composed_autograd_3d(sizes, ngp, B, nbc, kind, fields):
    from diffnet_amd import ops
    m = box_module(*sizes, ngp)
    shape = (B, 1, *sizes[::-1])
    u, lam = seeded(shape, 1, -0.5).to(dev()), seeded(shape, 2, -0.5).to(dev())
    nu, f = seeded(shape, 3, 0.5).to(dev()), seeded(shape, 4, -0.5).to(dev())
    dl = conditions(shape, B, 10, nbc, kind, fields)
    c, jac = 1.0, 0.8
    s = 1.0 / (B * m.geom.nelem_total)
    en, ef, rn, rf = reference_grads(m, u, nu, f, lam, dl, c, jac)
    g_nu, g_f = ops.poisson_coef_grad(m.geom, u, None, dl, s * c, -s, jac)
    gclose(g_nu, en, "energy d/dnu")
    gclose(g_f, ef, "energy d/df")
    g_nu, g_f = ops.poisson_coef_grad(m.geom, u, lam, dl, 1.0, -1.0, jac)
    gclose(g_nu, rn, "residual VJP d/dnu")
    gclose(g_f, rf, "residual VJP d/df")
    a = ops.poisson_coef_grad(m.geom, u, lam, dl, 1.0, -1.0, jac)
    assert torch.equal(a[0], g_nu) and torch.equal(a[1], g_f)
    alone = ops.poisson_coef_grad(m.geom, u[-1:].contiguous(), lam[-1:].contiguous(), [(mk[-1:] if mk.shape[0] == B else mk, v[-1:] if isinstance(v, torch.Tensor) else v)
                                                                                      for mk, v in dl], 1.0, -1.0, jac)
    assert torch.equal(alone[0], g_nu[-1:]) and torch.equal(alone[1], g_f[-1:])


# ---------------------------------------------------------------------------------------------
# 2. the reference's topology-optimisation losses
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["loss_topopt_n17.npz", "loss_topopt_n33.npz"])
def test_topopt_fixtures(name):
    z = np.load(os.path.join(GOLDEN, name))
    n = z["u"].shape[-1]
    m = module(dict(domain_size=n))
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    u, rho, f = cu(z["u"]).requires_grad_(True), cu(z["rho"]).requires_grad_(True), cu(z["f"])
    bc1, bc2 = cu(z["inputs"][:, 0:1]), cu(z["inputs"][:, 1:2])
    nu = 0.001 + torch.sigmoid(rho) ** 3
    L = m.energy_loss(u, nu, f, c=0.5)                        # the reference's Jacobian factor is the rule's weights alone
    gu, gr = torch.autograd.grad(L, (u, rho))
    np.testing.assert_allclose(float(L), float(z["loss"]) - float(z["dbc"]), rtol=LOSS_RTOL)
    gclose(gu, cu(z["loss_du"] - z["dbc_du"]), "loss d/du")
    gclose(gr, cu(z["loss_drho"]), "loss d/drho")
    dl = [(bc1, 1.0), (bc2, 0.0)]
    Cv = m.energy_loss(u, None, f, dirichlet=dl, c=0.0)
    gu, = torch.autograd.grad(Cv, u)
    np.testing.assert_allclose(float(Cv), float(z["compliance"]), rtol=LOSS_RTOL, atol=1e-7)
    gclose(gu, cu(z["compliance_du"]), "compliance d/du")
    # the optimiser-loop form gives the same three gradients from two launches
    loss, g = m.energy_loss_and_grads(u, nu, f, c=0.5)
    np.testing.assert_allclose(float(loss), float(z["loss"]) - float(z["dbc"]), rtol=LOSS_RTOL)
    sg = torch.sigmoid(rho.detach())
    gclose(g["nu"] * 3.0 * sg ** 3 * (1.0 - sg), cu(z["loss_drho"]), "energy_loss_and_grads d/drho")
    gclose(g["u"], cu(z["loss_du"] - z["dbc_du"]), "energy_loss_and_grads d/du")


# ---------------------------------------------------------------------------------------------
# 3. bitwise: runs, batch sizes, launch plans
# ---------------------------------------------------------------------------------------------
def test_bitwise_across_runs_batch_sizes_and_launch_plans():
    from diffnet_amd import _lib, ops
    nx, ny, B = 125, 77, 5
    m = rect_module(nx, ny, 3)
    shape = (B, 1, ny, nx)
    u, v = seeded(shape, 1, -0.5).to(dev()), seeded(shape, 2, -0.5).to(dev())
    nu, f = seeded(shape, 3, 0.5).to(dev()), seeded(shape, 4, -0.5).to(dev())
    mask = blob(shape, 5).to(dev()).to(torch.uint8)
    val = seeded(shape, 6, -0.5).to(dev())
    dl = [(mask, val)]

    def run(sel=slice(None)):
        """the raw launch with and without v, and energy_loss_and_grads"""
        d = [(mask[sel].contiguous(), val[sel].contiguous())]
        a = ops.poisson_coef_grad(m.geom, u[sel].contiguous(), v[sel].contiguous(), d, 0.7, -1.1, 0.4)
        b = ops.poisson_coef_grad(m.geom, u[sel].contiguous(), None, d, 0.7, -1.1, 0.4)
        loss, g = m.energy_loss_and_grads(u[sel].contiguous(), nu[sel].contiguous(), f[sel].contiguous(), dirichlet=d, c=0.5, jac=0.4)
        return [*a, *b, g["u"], g["nu"], g["f"]], loss

    base, loss0 = run()
    again, loss1 = run()
    assert all(torch.equal(x, y) for x, y in zip(base, again)) and torch.equal(loss0, loss1)
    for b in (0, 3):                                           # sample b of B = 5 equals the same sample alone (another launch plan)
        alone, _ = run(slice(b, b + 1))
        for k, (x, y) in enumerate(zip(base[:4], alone[:4])):
            assert torch.equal(x[b:b + 1], y), (b, k)
        for k in (5, 6):                                       # energy_loss_and_grads carries the loss scale 1 / (B nel) in a_nu, a_f: the sample
            gclose(alone[k], base[k][b:b + 1] * B)             # alone is B times larger, equal to rounding (B is no power of two), not bitwise
    try:
        for plan in ("64,2,8", "128,4,7", "64,2,5", "64,2,200"):         # (threads, elements per thread: the Poisson kernel's; R: both kernels')
            _lib.config_set("PLAN2D", plan)
            got, _ = run()
            for k in (0, 1, 2, 3, 5, 6):
                assert torch.equal(base[k], got[k]), (plan, k)
    finally:
        _lib.config_set("PLAN2D", "")


# ---------------------------------------------------------------------------------------------
# 4. two exact checks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,shape", [(dict(domain_size=65, ngp_1d=3), (2, 1, 65, 65)), (dict(nsd=3, domain_size=12), (1, 1, 12, 12, 12))])
def test_exact_constant_field_and_load_vector(kw, shape):
    from diffnet_amd import ops
    m = module(kw)
    const = torch.full(shape, 0.75, device=dev())
    g_nu, _ = ops.poisson_coef_grad(m.geom, const, None, (), 1.0, 1.0, 1.0)
    assert not g_nu.any()                                     # a constant u has no gradient: exactly zero
    one = torch.ones(shape, device=dev())
    _, g_f = ops.poisson_coef_grad(m.geom, one, None, (), 1.0, 1.0, 0.3)
    load, _ = ops.poisson_apply(m.geom, torch.zeros_like(one), None, one, None, (), alpha=0.0, beta=1.0, c=0.0, wscale=0.3, want_out=True, want_sums=False)
    gclose(g_f, -load, "g_f at u = 1 is the load vector of f = 1")
    np.testing.assert_allclose(float(g_f.double().sum()), 0.3 * 2.0 ** m.geom.nsd * m.geom.nelem_total * shape[0], rtol=LOSS_RTOL)


# ---------------------------------------------------------------------------------------------
# 5. routing
# ---------------------------------------------------------------------------------------------
class _Count:
    """counts the gauss_pt_eval launches of the composed route"""

    def __enter__(self):
        from diffnet_amd import ops
        self.ops, self.orig, self.n = ops, ops._GaussPtEval.apply, 0

        def counted(*a, **k):
            self.n += 1
            return self.orig(*a, **k)
        ops._GaussPtEval.apply = staticmethod(counted)
        return self

    def __exit__(self, *exc):
        self.ops._GaussPtEval.apply = staticmethod(self.orig)


@pytest.mark.parametrize("kw,shape", [(dict(domain_size=33, ngp_1d=3), (2, 1, 33, 33)), (dict(nsd=3, domain_size=9), (2, 1, 9, 9, 9))])
def test_routing_and_switch(kw, shape):
    from diffnet_amd import _lib, ops
    m = module(kw)
    u0, nu0, f0 = seeded(shape, 1, -0.5).to(dev()), seeded(shape, 2, 0.5).to(dev()), seeded(shape, 3, -0.5).to(dev())
    dl = [(boundary_mask(shape).to(dev()), 0.25)]

    def grads(fn):
        u, nu, f = (t.clone().requires_grad_(True) for t in (u0, nu0, f0))
        val = fn(u, nu, f)
        return [val.detach()] + list(torch.autograd.grad(val, (u, nu, f)))

    fns = {"energy": lambda u, nu, f: m.energy_loss(u, nu, f, dirichlet=dl, c=0.5, jac=0.6),
           "residual_loss": lambda u, nu, f: m.residual_loss(u, nu, f, dirichlet=dl, jac=0.6),
           "residual": lambda u, nu, f: (m.residual(u, nu, f, dirichlet=dl, jac=0.6) * f0).sum()}
    for name, fn in fns.items():
        before = ops._COEF_STATS["launch"]
        with _Count() as cnt:
            fused = grads(fn)
        assert cnt.n == 0 and ops._COEF_STATS["launch"] > before, name
        try:
            _lib.config_set("COEF_GRAD", "composed")
            with _Count() as cnt:
                comp = grads(fn)
        finally:
            _lib.config_set("COEF_GRAD", "")
        assert cnt.n > 0, name
        np.testing.assert_allclose(float(fused[0]), float(comp[0]), rtol=LOSS_RTOL, err_msg=name)
        for a, b, what in zip(fused[1:], comp[1:], ("u", "nu", "f")):
            gclose(a, b, f"{name} d/d{what}")
    # a Dirichlet value field or an f_gp that requires a gradient keeps the composed route, and gets its gradient
    val = seeded(shape, 5, -0.5).to(dev()).requires_grad_(True)
    nu = nu0.clone().requires_grad_(True)
    with _Count() as cnt:
        m.energy_loss(u0, nu, f0, dirichlet=[(dl[0][0], val)], c=0.5).backward()
    assert cnt.n > 0 and val.grad.abs().max() > 0 and nu.grad.abs().max() > 0
    f_gp = seeded((shape[0], m.geom.ngp_total, *m.geom.elem_shape), 6, -0.5).to(dev()).requires_grad_(True)
    with _Count() as cnt:
        m.energy_loss(u0, nu0, None, f_gp=f_gp, dirichlet=dl, c=0.5).backward()
    assert cnt.n > 0 and f_gp.grad.abs().max() > 0
    # ... while an f_gp that does not is no obstacle to the fused nu gradient
    nu = nu0.clone().requires_grad_(True)
    with _Count() as cnt:
        m.energy_loss(u0, nu, None, f_gp=f_gp.detach(), dirichlet=dl, c=0.5).backward()
    assert cnt.n == 0 and nu.grad.abs().max() > 0


# ---------------------------------------------------------------------------------------------
# 6. Hessian-vector product
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,shape", [(dict(domain_size=33), (2, 1, 33, 33)), (dict(nsd=3, domain_size=9), (1, 1, 9, 9, 9))])
def test_hessian_vector_product_matches_composed_double_backward(kw, shape):
    from diffnet_amd import ops
    m = module(kw)
    u0, nu0, f0 = seeded(shape, 1, -0.5).to(dev()), seeded(shape, 2, 0.5).to(dev()), seeded(shape, 3, -0.5).to(dev())
    wu, wn = seeded(shape, 4, -0.5).to(dev()), seeded(shape, 5, -0.5).to(dev())
    dl = [(boundary_mask(shape).to(dev()), 0.25)]

    def hvp(fn):
        u, nu = u0.clone().requires_grad_(True), nu0.clone().requires_grad_(True)
        gu, gn = torch.autograd.grad(fn(u, nu), (u, nu), create_graph=True)
        return torch.autograd.grad((gu * wu).sum() + (gn * wn).sum(), (u, nu))

    with _Count() as cnt:
        fu, fn_ = hvp(lambda u, nu: m.energy_loss(u, nu, f0, dirichlet=dl, c=0.5, jac=0.6))
    assert cnt.n == 0
    cu_, cn = hvp(lambda u, nu: ops.composed_energy(m.geom, u, nu, f0, None, dl, 0.5, 0.6))
    gclose(fu, cu_, "H (wu, wn) wrt u")
    gclose(fn_, cn, "H (wu, wn) wrt nu")
    # and through the residual loss (v present in the coefficient launch)
    fu, fn_ = hvp(lambda u, nu: m.residual_loss(u, nu, f0, dirichlet=dl, jac=0.6))
    cu_, cn = hvp(lambda u, nu: (ops.composed_residual(m.geom, u, nu, f0, None, dl, 0.6) ** 2).sum())
    gclose(fu, cu_, "residual_loss H wrt u")
    gclose(fn_, cn, "residual_loss H wrt nu")


# ---------------------------------------------------------------------------------------------
# 7. isolation and capture
# ---------------------------------------------------------------------------------------------
def test_coefficient_launch_between_chained_launches_changes_nothing():
    from diffnet_amd import ops
    # FSDT defer_norms -> norms_from
    m = module(dict(domain_size=129, fem_basis_deg=2, ngp_1d=3))
    shape = (2, 1, 129, 129)
    flds = [seeded(shape, 100 + i).to(dev()) for i in range(3)]
    bcm = boundary_mask(shape).to(dev())
    consts = dict(D11=1.3, D12=0.4, D22=1.1, D66=0.6, A44=0.8, A55=0.9, q=1.2, wscale=0.3)
    wts = torch.tensor([1.0, 0.5, 2.0], device=dev())
    pm = module(dict(domain_size=257, ngp_1d=3))
    pshape = (4, 1, 257, 257)
    pu, pv = seeded(pshape, 7).to(dev()), seeded(pshape, 8).to(dev())
    pbc = boundary_mask(pshape).to(dev()).to(torch.uint8)

    def coef():
        ops.poisson_coef_grad(pm.geom, pu, pv, [(pbc, 0.0)], 1.0, -1.0, 1.0)
        ops.poisson_coef_grad(pm.geom, pu, None, [(pbc, 0.0)], 1.0, -1.0, 1.0)

    def pair(interleave):
        Rs, _, h = ops.fsdt_apply(m.geom, *flds, bcm, want_sums=False, defer_norms=True, **consts)
        if interleave:
            coef()
        g, _, n = ops.fsdt_apply(m.geom, *Rs, bcm, want_sums=False, want_norms=True, in_num=wts, norms_from=h, **dict(consts, q=0.0))
        return g, n

    g0, n0 = pair(False)
    g1, n1 = pair(True)
    assert torch.equal(n0, n1) and all(torch.equal(a, b) for a, b in zip(g0, g1)) and not torch.isnan(n1).any()
    # chained Poisson fold_prev launches
    B = 4
    scale = 1.0 / (B * pm.geom.nelem_total)
    kwargs = dict(alpha=2.0, beta=1.0, c=1.0, wscale=1.0, out_scale=scale, want_out=True, want_sums=True, loss_scale=scale)
    sets = [(seeded(pshape, 20 + 3 * k).to(dev()), seeded(pshape, 21 + 3 * k, 0.5).to(dev()), seeded(pshape, 22 + 3 * k).to(dev())) for k in range(2)]

    def chain(interleave):
        plans = [ops.PoissonPlan(pm.geom, *s, None, [(pbc, 0.0)], pipelined_sums=True, **kwargs) for s in sets]
        plans[1].fold(plans[0])
        plans[0].launch()
        if interleave:
            coef()
        plans[1].launch()
        if interleave:
            coef()
        plans[1].finish_sums()
        return [t.clone() for p in plans for t in p.result]

    for a, b in zip(chain(False), chain(True)):
        assert torch.equal(a, b)


def test_energy_loss_and_grads_replays_bitwise_in_a_hip_graph():
    m = rect_module(125, 41, 3)
    shape = (3, 1, 41, 125)
    u, nu, f = seeded(shape, 1, -0.5).to(dev()), seeded(shape, 2, 0.5).to(dev()), seeded(shape, 3, -0.5).to(dev())
    dl = [(boundary_mask(shape).to(dev()), 0.25)]
    loss0, g0 = m.energy_loss_and_grads(u, nu, f, dirichlet=dl, c=0.5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.energy_loss_and_grads(u, nu, f, dirichlet=dl, c=0.5)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, g = m.energy_loss_and_grads(u, nu, f, dirichlet=dl, c=0.5)
    for _ in range(2):
        loss.fill_(-1.0)
        for t in g.values():
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, loss0) and all(torch.equal(g[k], g0[k]) for k in ("u", "nu", "f"))


# ---------------------------------------------------------------------------------------------
# 8. full size: size-independent properties
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,shape", [(dict(domain_size=512), (64, 1, 512, 512)), (dict(domain_size=2049), (2, 1, 2049, 2049)),
                                      (dict(nsd=3, domain_size=128), (1, 1, 128, 128, 128))])
def test_full_size_properties(kw, shape):
    from diffnet_amd import ops
    m = module(kw)
    u = seeded(shape, 1, -0.5).to(dev())
    mu, d = seeded(shape, 2, 0.5).to(dev()), seeded(shape, 3, 0.5).to(dev())
    dl = [(boundary_mask(shape).to(dev()).to(torch.uint8), 0.25)]
    g_nu, g_f = ops.poisson_coef_grad(m.geom, u, None, dl, 1.0, 1.0, 1.0)
    again = ops.poisson_coef_grad(m.geom, u, None, dl, 1.0, 1.0, 1.0)
    assert torch.equal(g_nu, again[0]) and torch.equal(g_f, again[1])
    # <mu, g_nu(u~)> = <u~, K_mu u~> = the stiffness energy with coefficient mu, from the existing operator
    _, sums = ops.poisson_apply(m.geom, u, mu, None, None, dl, alpha=1.0, beta=0.0, c=1.0, wscale=1.0, want_out=False, want_sums=True)
    np.testing.assert_allclose(float((mu.double() * g_nu.double()).sum()), float(sums[0]), rtol=LOSS_RTOL)
    # the energy is linear in nu: E(nu + d) - E(nu) = <d, dE/dnu>
    _, s1 = ops.poisson_apply(m.geom, u, mu + d, None, None, dl, alpha=1.0, beta=0.0, c=1.0, wscale=1.0, want_out=False, want_sums=True)
    np.testing.assert_allclose(float(s1[0]) - float(sums[0]), float((d.double() * g_nu.double()).sum()), rtol=GRAD_RTOL)


# ---------------------------------------------------------------------------------------------
# 9. the example, both modes, in fresh processes
# ---------------------------------------------------------------------------------------------
def test_topopt_example_agrees_between_modes(tmp_path):
    out = {}
    for mode in ("fused", "composed"):
        path = str(tmp_path / f"{mode}.pt")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "topopt_2d.py"), "--size", "33", "--epochs", "4", "--mode", mode,
                            "--dump", path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.count("energy") == 4
        out[mode] = torch.load(path)
    for k in ("u", "rho"):
        gclose(out["fused"][k], out["composed"][k], k)
    np.testing.assert_allclose(out["fused"]["values"], out["composed"]["values"], rtol=GRAD_RTOL)
