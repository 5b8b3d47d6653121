"""GPU tests of the fused 2-D scalar transport (SUPG) residual (dn_transport_apply, csrc/transport.hip; diffnet_amd/transport.py): against
the reference fixtures (tests/golden/loss_transport_*.npz, the reference scripts' own `loss` bodies), against the same residual composed
from the drop-in operators on every compile-time form and on ragged meshes around the wave's 62-column chunk, the VJP launch against
autograd through the composition, the adjoint identity of the linear cases, bitwise independence of batch and launch plan, the Dirichlet
rows, the tie to the Poisson operator, isolation of its reduction workspace from the other operators' launches, graph capture, the full
size, and the example."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import boundary_mask, close, cu, dev, load, module, seeded
from test_transport_host import FIXTURES, GRAD_AREL, GRAD_RTOL, LOSS_RTOL, fixture_case, transport_torch

pytestmark = pytest.mark.gpu

E17 = dict(adv=(0.8660254, 0.5), kappa=(0.01, 0.01), tau=0.02, react=(0.0, 0.0, 0.0, 0.0))
E3 = dict(adv=(0.0, 1.0), kappa=(0.3, 0.0), tau=0.015, react=(0.0, 0.0, 0.0, 0.0), r_first_wins=True)
E18 = dict(adv=(0.0, 1.0), kappa=(0.04, 0.04), tau=0.0, react=(-8.0, 32.0, -96.0, 64.0))
# nx around the 62 owner columns of a wave (one chunk, one chunk + 1, two, three + 1), ny around the shortest strip (8 rows)
SHAPES = [(2, 2, 1, 2), (3, 9, 3, 3), (62, 8, 8, 2), (63, 17, 1, 4), (64, 5, 3, 2), (125, 33, 8, 3), (187, 70, 3, 2), (64, 300, 1, 2)]


def fixture_inputs(z):
    c = fixture_case(z)
    m = module(eval(str(z["kwargs"])))
    f32 = lambda a: cu(np.asarray(a, dtype=np.float32))                    # noqa: E731
    inp = cu(z["inputs"])
    v1 = f32(c["vals"][0]).reshape(1, 1, *inp.shape[-2:]) if np.ndim(c["vals"][0]) else float(c["vals"][0])
    kw = dict(bc=(inp[:, 1:2].contiguous(), inp[:, 2:3].contiguous()), bc_values=(v1, 0.0), nu=inp[:, 0:1].contiguous() if c["nu"] is not None else None,
              f_gp=f32(c["f"]), adv=c["adv"], kappa=c["kappa"], tau=c["tau"], react=c["react"], wscale=c["J"], r_first_wins=c["first"])
    return m, kw


@pytest.mark.parametrize("name", FIXTURES)
def test_transport_vs_reference_golden(name):
    from diffnet_amd.transport import transport_loss, transport_loss_and_grad
    z = load(name)
    m, kw = fixture_inputs(z)
    u = cu(z["u"]).requires_grad_(True)
    loss = transport_loss(m, u, **kw)
    g, = torch.autograd.grad(loss, u)
    ref = z["grad"]
    print(name, "loss rel", abs(float(loss) - float(z["loss"])) / float(z["loss"]), "grad", float(np.abs(g.cpu().numpy() - ref).max() / np.abs(ref).max()))
    np.testing.assert_allclose(float(loss), float(z["loss"]), rtol=LOSS_RTOL)
    close(g, ref, rtol=GRAD_RTOL, arel=GRAD_AREL)
    l2, g2 = transport_loss_and_grad(m, u.detach(), **kw)
    np.testing.assert_allclose(float(l2), float(z["loss"]), rtol=LOSS_RTOL)
    close(g2, ref, rtol=GRAD_RTOL, arel=GRAD_AREL)


def rect_module(nx, ny, ngp, lengths=(1.0, 0.7)):
    return module(dict(domain_sizes=(nx, ny), domain_lengths=lengths, domain_size=nx, domain_length=lengths[0], ngp_1d=ngp))


def _max_rel(a, b):
    scale = max(float(b.abs().max()), float(a.abs().max()), 1e-30)
    return float((a - b).abs().max()) / scale


def _cases(shape, ngp):
    """(name, bc, bc_values, nu, f_gp, coefficients): every compile-time form (mask none / constants / value fields, nu, Gauss-point
    forcing, reaction) at least once; masks fp32 / uint8 / bool, shared and per sample"""
    B, _, ny, nx = shape
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(3)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float())
    shared = wall[:1].contiguous()
    G, eshape = ngp * ngp, (ny - 1, nx - 1)
    f_sh = cu(seeded((G, *eshape), 20, -0.5)) * 4.0
    f_b = cu(seeded((B, G, *eshape), 21, -0.5)) * 4.0
    vfield = cu(seeded(shape, 30, -0.5))
    vshared = cu(seeded((1, 1, ny, nx), 31, -0.5))
    nu_b = cu(seeded(shape, 32, 0.5))
    nu_sh = cu(seeded((1, 1, ny, nx), 33, 0.5))
    return [
        ("no masks, constant forcing, linear", None, (0.0, 0.0), None, 0.7, E17),
        ("no masks, nu, gp forcing, reaction", None, (0.0, 0.0), nu_sh, f_b, E18),
        ("fp32 shared + per sample, constants, nu per sample", (shared, blob), (1.0, 0.0), nu_b, None, E17),
        ("fp32 overlapping, value fields, gp forcing shared, first wins", (wall, blob), (vfield, vshared), None, f_sh, E3),
        ("u8 per sample + bool shared, value field + constant, reaction", (blob.to(torch.uint8), shared.bool()), (vshared, 0.25), None, f_sh, E18),
        ("bool only condition 2, nu, reaction, constant forcing", (None, blob.bool()), (0.0, -0.4), nu_sh, -1.3, E18),
        ("u8 shared, value field per sample, nu, gp forcing per sample", (shared.to(torch.uint8), None), (vfield, 0.0), nu_b, f_b, E17),
    ]


# Tolerance 1e-4 of the largest residual, as the Navier-Stokes tests: the two implementations round the products of the weak form in
# different orders.  The cubic with coefficients up to 64 on |u| <= 1 stays inside it (the measured distances are printed).
@pytest.mark.parametrize("nx,ny,B,ngp", SHAPES)
def test_transport_fused_matches_composed(nx, ny, B, ngp):
    from diffnet_amd.transport import transport_loss, transport_residual, transport_residual_composed
    m = rect_module(nx, ny, ngp)
    shape = (B, 1, ny, nx)
    u = cu(seeded(shape, 10, -0.5)) * 2.0
    for name, bc, vals, nu, f, coef in _cases(shape, ngp):
        kw = dict(bc=bc, bc_values=vals, nu=nu, f_gp=f, **coef)
        ua, ub = u.clone().requires_grad_(True), u.clone().requires_grad_(True)
        got, ref = transport_residual(m, ua, **kw), transport_residual_composed(m, ub, **kw)
        d = _max_rel(got, ref)
        la, lb = transport_loss(m, ua, **kw), (ref ** 2).sum()
        ga, = torch.autograd.grad(la, ua)
        gb, = torch.autograd.grad(lb, ub)
        print((nx, ny, B, ngp), name, "R", d, "loss", abs(float(la) - float(lb)) / max(float(lb), 1e-30), "grad", _max_rel(ga, gb))
        assert d <= 1e-4, (name, d)
        np.testing.assert_allclose(float(la), float(lb), rtol=2e-5, atol=1e-30, err_msg=name)
        assert _max_rel(ga, gb) <= 1e-4, (name, "gradient", _max_rel(ga, gb))
        na = transport_loss(m, ua, kind="norm", **kw)
        np.testing.assert_allclose(float(na), float(lb) ** 0.5, rtol=2e-5, atol=1e-30, err_msg=name)


@pytest.mark.parametrize("nx,ny,B,ngp", SHAPES[1:])
def test_transport_vjp_launch_matches_autograd_of_composed(nx, ny, B, ngp):
    from diffnet_amd.transport import transport_loss, transport_residual, transport_residual_composed
    m = rect_module(nx, ny, ngp)
    shape = (B, 1, ny, nx)
    u = cu(seeded(shape, 40, -0.5)) * 2.0
    cot = cu(seeded(shape, 50, -0.5))
    for name, bc, vals, nu, f, coef in _cases(shape, ngp):
        kw = dict(bc=bc, bc_values=vals, nu=nu, f_gp=f, **coef)
        ua, ub = u.clone().requires_grad_(True), u.clone().requires_grad_(True)
        ga, = torch.autograd.grad(transport_residual(m, ua, **kw), ua, cot)
        gb, = torch.autograd.grad(transport_residual_composed(m, ub, **kw), ub, cot)
        assert _max_rel(ga, gb) <= 1e-4, (name, "cot", _max_rel(ga, gb))
        na = transport_loss(m, ua, kind="norm", **kw)
        nb = torch.norm(transport_residual_composed(m, ub, **kw))
        ga, = torch.autograd.grad(na, ua)
        gb, = torch.autograd.grad(nb, ub)
        assert _max_rel(ga, gb) <= 1e-4, (name, "norm", _max_rel(ga, gb))
        # no gradient reaches a Dirichlet node
        masks = [mk for mk in ((None, None) if bc is None else bc) if mk is not None]
        for mk in masks:
            fixed = (mk != 0) if mk.dtype != torch.float32 else (mk >= 0.5)
            assert float((ga * fixed.expand_as(ga)).abs().max()) == 0.0, name


@pytest.mark.parametrize("coef", [E17, E3], ids=["e17", "e3"])
def test_transport_linear_cases_satisfy_the_adjoint_identity(coef):
    """<J x, y> = <x, J^T y>: J x as the difference of two forward launches (the operator is affine in u), J^T y from the VJP launch."""
    from diffnet_amd import ops
    m = rect_module(125, 47, 3)
    shape = (2, 1, 47, 125)
    wall = boundary_mask(shape).to(dev())
    nu = cu(seeded(shape, 61, 0.5))
    kw = dict(nu=nu, bc=(wall, None), bc_values=(0.3, 0.0), f_gp=0.4, wscale=1.0, **coef)
    x, y, u0 = (cu(seeded(shape, 62 + i, -0.5)) for i in range(3))
    r1, _ = ops.transport_apply(m.geom, u0 + x, want_sums=False, **kw)
    r0, _ = ops.transport_apply(m.geom, u0, want_sums=False, **kw)
    jty, _ = ops.transport_apply(m.geom, u0, cot=y, want_sums=False, **kw)
    free = (wall < 0.5).double()
    lhs = float((((r1 - r0).double() * y.double()) * free).sum())          # the Dirichlet rows of R are constants
    rhs = float((x.double() * jty.double()).sum())
    np.testing.assert_allclose(lhs, rhs, rtol=1e-4)


def test_transport_bitwise_across_batch_sizes_plans_and_runs():
    from diffnet_amd import ops
    m = rect_module(187, 129, 2)
    B = 8
    shape = (B, 1, 129, 187)
    u, cot = cu(seeded(shape, 70, -0.5)), cu(seeded(shape, 71, -0.5))
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(9)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float())
    vals = (cu(seeded(shape, 80, -0.5)), 0.2)
    nu = cu(seeded(shape, 82, 0.5))
    f = cu(seeded((B, 4, 128, 186), 81, -0.5))
    kw = dict(wscale=0.2, **E18)
    out, sums = ops.transport_apply(m.geom, u, nu, (wall, blob.to(torch.uint8)), vals, f_gp=f, **kw)
    grad, _ = ops.transport_apply(m.geom, u, nu, (wall, blob.to(torch.uint8)), vals, f_gp=f, cot=cot, want_sums=False, **kw)
    out2, sums2 = ops.transport_apply(m.geom, u, nu, (wall, blob.to(torch.uint8)), vals, f_gp=f, **kw)
    assert torch.equal(out, out2) and torch.equal(sums, sums2)                  # run to run
    np.testing.assert_allclose(float(sums), float((out.double() ** 2).sum()), rtol=1e-6)
    # a smaller batch takes another launch plan (more, shorter strips): the same bits
    for sl in (slice(0, 1), slice(5, 6), slice(2, 5)):
        one = lambda t: t[sl].contiguous()                                      # noqa: E731
        ob, _ = ops.transport_apply(m.geom, one(u), one(nu), (one(wall), one(blob).to(torch.uint8)), (one(vals[0]), 0.2), f_gp=one(f), want_sums=False, **kw)
        gb, _ = ops.transport_apply(m.geom, one(u), one(nu), (one(wall), one(blob).to(torch.uint8)), (one(vals[0]), 0.2), f_gp=one(f), cot=one(cot),
                                    want_sums=False, **kw)
        assert torch.equal(out[sl], ob) and torch.equal(grad[sl], gb), sl


def test_transport_dirichlet_rows_take_the_values_and_overlap_rule():
    from diffnet_amd.transport import transport_residual
    m = rect_module(64, 20, 2)
    shape = (2, 1, 20, 64)
    u = cu(seeded(shape, 90, -0.5))
    m1 = torch.zeros(shape)
    m1[..., 0, :] = 1.0
    m2 = torch.zeros(shape)
    m2[..., :, 0] = 1.0
    m2[..., :, -1] = 1.0
    m1, m2 = m1.to(dev()), m2.to(dev())
    v1 = cu(seeded(shape, 91, 0.5))
    only1, only2, both = (m1 > 0.5) & (m2 < 0.5), (m2 > 0.5) & (m1 < 0.5), (m1 > 0.5) & (m2 > 0.5)
    for first in (False, True):
        R = transport_residual(m, u, (m1, m2), (v1, -0.75), r_first_wins=first, **E17)
        assert torch.equal(R[only1], v1[only1]) and bool((R[only2] == -0.75).all())
        assert torch.equal(R[both], v1[both]) if first else bool((R[both] == -0.75).all())
    # on u condition 2 always wins: the residual off the Dirichlet rows does not depend on r_first_wins, and moves with value 2
    Ra = transport_residual(m, u, (m1, m2), (v1, -0.75), r_first_wins=False, **E17)
    Rb = transport_residual(m, u, (m1, m2), (v1, -0.75), r_first_wins=True, **E17)
    free = (m1 < 0.5) & (m2 < 0.5)
    assert torch.equal(Ra[free], Rb[free])
    ref = transport_torch(u[0, 0].double().cpu(), None, [m1[0, 0].cpu() > 0.5, m2[0, 0].cpu() > 0.5], [v1[0, 0].double().cpu().numpy(), -0.75], 0.0,
                          E17["adv"], E17["kappa"], E17["tau"], E17["react"], (0.5 * m.hx) * (0.5 * m.hy), m.hx, m.hy, 2, False)
    assert _max_rel(Ra[0, 0].double().cpu(), ref) <= 1e-4


@pytest.mark.parametrize("ngp", [2, 3])
def test_transport_without_transport_is_the_poisson_residual(ngp):
    """adv = 0, tau = 0, react = 0, kappa = (1, 1): the weak Poisson residual of fem.residual on the same u, nu, f off the Dirichlet rows"""
    from diffnet_amd.transport import transport_residual
    m = rect_module(125, 70, ngp)
    shape = (3, 1, 70, 125)
    u, nu = cu(seeded(shape, 95, -0.5)), cu(seeded(shape, 96, 0.5))
    f = cu(seeded((3, ngp * ngp, 69, 124), 97, -0.5))
    wall = boundary_mask(shape).to(dev())
    J = (0.5 * m.hx) * (0.5 * m.hy)
    R = transport_residual(m, u, (wall, None), (0.3, 0.0), nu=nu, f_gp=f, adv=(0.0, 0.0), kappa=(1.0, 1.0), tau=0.0)
    P = m.residual(u, nu, f_gp=f, dirichlet=[(wall, 0.3)], jac=J)
    free = wall < 0.5
    assert float(P[free].abs().max()) > 0
    assert _max_rel(R[free], P[free]) <= 1e-4, _max_rel(R[free], P[free])
    assert bool((R[~free] == 0.3).all())


def _neighbours():
    """reducing launches of the other operators on meshes of their own"""
    from diffnet_amd import ops
    shape = (2, 1, 129, 129)
    sm = module(dict(domain_size=129))
    sf = [cu(seeded(shape, 110 + i, -0.5)) for i in range(3)]
    bcm = boundary_mask(shape).to(dev())
    nu = cu(seeded(shape, 114, 0.5))

    def poisson():
        return sm.energy_loss_and_grad(sf[0], nu, sf[1], dirichlet=[(bcm, 0.0)])

    def stokes():
        return ops.stokes_apply(sm.geom, *sf, bcm, (0.1, 0.0, 0.0), 0.7, 0.01, (0.2, 0.1), 0.25, want_norms=True)

    def ns():
        return ops.ns_apply(sm.geom, *sf, bcm, (0.1, 0.0, 0.0), 0.05, (0.2, 0.1), 0.25, want_norms=True)

    return dict(poisson=poisson, stokes=stokes, ns=ns)


def _flat(r):
    out = []
    for x in (r if isinstance(r, (tuple, list)) else [r]):
        out += _flat(x) if isinstance(x, (tuple, list)) else ([] if x is None else [x])
    return out


def test_transport_chained_with_the_other_operators_on_one_stream():
    """Transport launches between Poisson / Stokes / NS launches, both orders: nobody's sums or outputs change."""
    from diffnet_amd import ops
    m = rect_module(187, 129, 2)
    shape = (2, 1, 129, 187)
    u = cu(seeded(shape, 120, -0.5))
    wall = boundary_mask(shape).to(dev())

    def tr():
        return ops.transport_apply(m.geom, u, None, (wall, None), (1.0, 0.0), f_gp=0.3, want_norm=True, **E18)

    others = _neighbours()
    ref_t = _flat(tr())
    refs = {k: _flat(fn()) for k, fn in others.items()}
    seq = []
    for k, fn in others.items():
        seq += [("t", tr()), (k, fn()), ("t", tr()), (k, fn()), (k, fn()), ("t", tr())]
    torch.cuda.synchronize()
    for k, r in seq:
        for a, b in zip(_flat(r), ref_t if k == "t" else refs[k]):
            assert torch.equal(a, b), k


def test_transport_launch_between_fsdt_defer_and_consumer_changes_nothing():
    from diffnet_amd import ops
    m = module(dict(domain_size=129, fem_basis_deg=2, ngp_1d=3))
    shape = (2, 1, 129, 129)
    flds = [cu(seeded(shape, 100 + i)) for i in range(3)]
    bcm = boundary_mask(shape).to(dev())
    consts = dict(D11=1.3, D12=0.4, D22=1.1, D66=0.6, A44=0.8, A55=0.9, q=1.2, wscale=0.3)
    wts = torch.tensor([1.0, 0.5, 2.0], device=dev())
    tm = module(dict(domain_size=129))
    tu = cu(seeded(shape, 113, -0.5))
    t_ref = ops.transport_apply(tm.geom, tu, None, (bcm, None), (1.0, 0.0), f_gp=0.3, want_norm=True, **E17)

    def pair(interleave):
        Rs, _, h = ops.fsdt_apply(m.geom, *flds, bcm, want_sums=False, defer_norms=True, **consts)
        t = ops.transport_apply(tm.geom, tu, None, (bcm, None), (1.0, 0.0), f_gp=0.3, want_norm=True, **E17) if interleave else None
        g, _, n = ops.fsdt_apply(m.geom, *Rs, bcm, want_sums=False, want_norms=True, in_num=wts, norms_from=h, **dict(consts, q=0.0))
        return g, n, t

    g0, n0, _ = pair(False)
    g1, n1, t1 = pair(True)
    assert torch.equal(n0, n1) and torch.isfinite(n1).all()
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    for a, b in zip(t1, t_ref):
        assert torch.equal(a, b)


def test_transport_loss_and_grad_graph_capture_replays_bitwise():
    from diffnet_amd.transport import transport_loss_and_grad
    m = rect_module(130, 47, 2)
    shape = (2, 1, 47, 130)
    u = cu(seeded(shape, 130, -0.5))
    wall = boundary_mask(shape).to(dev())
    kw = dict(bc=(wall, wall[:1].to(torch.uint8)), bc_values=(cu(seeded((1, 1, 47, 130), 134, -0.5)), 0.0), nu=cu(seeded(shape, 136, 0.5)),
              f_gp=cu(seeded((4, 46, 129), 135, -0.5)), **E18)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):                     # warm-up on the capture stream: workspace, prepared calls, the cached scale
            eager = transport_loss_and_grad(m, u, **kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            static = transport_loss_and_grad(m, u, **kw)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static[0], eager[0]) and torch.equal(static[1], eager[1])
    with torch.no_grad():
        u.mul_(0.5)                            # replays read the field in place
    g.replay()
    again = transport_loss_and_grad(m, u, **kw)
    torch.cuda.synchronize()
    assert torch.equal(static[0], again[0]) and torch.equal(static[1], again[1]) and not torch.equal(static[0], eager[0])


def test_transport_full_size_properties():
    """2049^2 B = 8 (no oracle at that size): the sum against the written residual, Dirichlet rows and gradient, bitwise equality with the
    same samples launched alone (another launch plan), repeatability."""
    from diffnet_amd import ops
    n, B = 2049, 8
    m = module(dict(domain_size=n))
    shape = (B, 1, n, n)
    u = cu(seeded(shape, 140, -0.5))
    wall = boundary_mask((1, 1, n, n)).to(dev()).to(torch.uint8)
    J = (0.5 * m.hx) * (0.5 * m.hy)
    for coef in (E17, E18):
        kw = dict(wscale=J, **coef)
        R, sums, norm = ops.transport_apply(m.geom, u, None, (wall, None), (1.0, 0.0), f_gp=0.3, want_norm=True, **kw)
        np.testing.assert_allclose(float(sums), float((R.double() ** 2).sum()), rtol=1e-6)
        np.testing.assert_allclose(float(norm), float(sums) ** 0.5, rtol=1e-6)
        fixed = (wall != 0).expand(shape)
        assert bool((R[fixed] == 1.0).all()) and torch.isfinite(R).all()
        g, _ = ops.transport_apply(m.geom, u, None, (wall, None), (1.0, 0.0), f_gp=0.3, cot=R, want_sums=False, **kw)
        assert float(g[fixed].abs().max()) == 0.0 and torch.isfinite(g).all() and float(g.abs().max()) > 0
        R2, sums2 = ops.transport_apply(m.geom, u, None, (wall, None), (1.0, 0.0), f_gp=0.3, **kw)
        assert torch.equal(R, R2) and torch.equal(sums, sums2)
        u1 = u[3:4].contiguous()
        R1, _ = ops.transport_apply(m.geom, u1, None, (wall, None), (1.0, 0.0), f_gp=0.3, want_sums=False, **kw)
        g1, _ = ops.transport_apply(m.geom, u1, None, (wall, None), (1.0, 0.0), f_gp=0.3, cot=R[3:4].contiguous(), want_sums=False, **kw)
        assert torch.equal(R[3:4], R1) and torch.equal(g[3:4], g1)


def test_transport_no_silent_zero_gradients_and_errors():
    from diffnet_amd import ops
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd.transport import transport_loss, transport_residual
    m = module(dict(domain_size=17))
    u = cu(seeded((1, 1, 17, 17), 1, -0.5))
    wall = boundary_mask((1, 1, 17, 17)).to(dev())
    nu = cu(seeded((1, 1, 17, 17), 2, 0.5)).requires_grad_(True)
    f = cu(seeded((4, 16, 16), 3, -0.5)).requires_grad_(True)
    v1 = cu(seeded((1, 1, 17, 17), 4, -0.5)).requires_grad_(True)
    loss = transport_loss(m, u.clone().requires_grad_(True), (wall, None), (v1, 0.0), nu=nu, f_gp=f, **E17)
    gs = torch.autograd.grad(loss, (nu, f, v1))
    assert all(float(g.abs().max()) > 0 for g in gs)
    m2 = module(dict(domain_size=17, fem_basis_deg=2))
    with pytest.raises(DiffNetHipError):
        transport_residual(m2, u)
    with pytest.raises(DiffNetHipError):
        transport_residual(m, u, (boundary_mask((1, 1, 17, 17)), None))            # a CPU mask
    with pytest.raises(ValueError):
        ops.transport_apply(m.geom, u, in_num=u[0, 0, 0, :1].contiguous())          # scaling without a VJP
    with pytest.raises(ValueError):
        ops.transport_apply(m.geom, u, None, (None, None), (v1.detach(), 0.0))      # a value field without its mask


def test_transport_example_fused_and_composed_agree():
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("ex_transport_2d", os.path.join(here, "..", "examples", "transport_2d.py"))
    ex = importlib.util.module_from_spec(spec)
    sys.modules["ex_transport_2d"] = ex
    spec.loader.exec_module(ex)
    for case in ("advdiff", "stheat", "allencahn"):
        _, hf = ex.run(case=case, size=33, steps=15, verbose=False, mode="fused")
        _, hc = ex.run(case=case, size=33, steps=15, verbose=False, mode="composed")
        np.testing.assert_allclose(np.array(hf), np.array(hc), rtol=1e-3, err_msg=case)
        assert hf[-1] < hf[0], case
