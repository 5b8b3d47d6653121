"""GPU tests of the fused 2-D eikonal weak-form residual and its VJP (dn_eikonal_apply, csrc/eikonal.hip; diffnet_amd/eikonal.py): against
the reference fixtures (tests/golden/loss_eikonal_*.npz, the reference script's own loss body), against the same functions composed from
the drop-in operators on every compile-time form, degree and rule, on ragged meshes around the march's seams; the VJP launch with a
random cotangent, the Dirichlet nodes, bitwise independence of batch and launch plan, isolation of its reduction workspace from a
Helmholtz launch, graph capture, gradient routing and the example."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from test_eikonal_host import FIXTURES, fixture_case
from test_gpu_helmholtz import SHAPES, LENGTHS, _fixed, _max_rel, hh_module
from test_gpu_parity import boundary_mask, close, cu, dev, load, module, seeded
from test_transport_host import GRAD_AREL, GRAD_RTOL, LOSS_RTOL

pytestmark = pytest.mark.gpu

# SHAPES: the meshes (degree, ngp, nelx, nely, B) of tests/test_gpu_helmholtz.py, which explains them: nelx around the 63 element columns
# of a one-wave chunk (1, 2, 62, 63, 64, 127) and 510, two chunks of the widest workgroup; nely around the shortest strip of 4 (1, 3, 4,
# 5, 14); every (degree, rule) pair once.
# The tolerances of the transport tests (tests/test_gpu_transport.py): R within 1e-4 of its largest entry, the loss within 2e-5 relative,
# the gradient within 1e-4 of its largest entry.
# Largest distances measured over all meshes and cases (the test prints each): R 1.3e-5, loss 2.5e-7 (norm) / 5.6e-7 (sumsq), gradient 1.3e-5,
# VJP with a random cotangent 1.0e-5.
RTOL_R, RTOL_LOSS, RTOL_G = 1e-4, 2e-5, 1e-4


def field(shape, seed, lengths=LENGTHS):
    """The fixtures' scaling: the distance to a circle (|grad u| = 1) + h x seeded noise in (-1/2, 1/2), h the node spacing along x"""
    B, _, ny, nx = shape
    x, y = torch.linspace(0, lengths[0], nx), torch.linspace(0, lengths[1], ny)
    r = torch.hypot(x[None, :] - 0.5 * lengths[0], y[:, None] - 0.5 * lengths[1]) - 0.3
    h = lengths[0] / max(nx - 1, 1)
    return cu(r + h * (seeded(shape, seed) - 0.5))


@pytest.mark.parametrize("name", FIXTURES)
def test_eikonal_vs_reference_golden(name):
    from diffnet_amd.eikonal import eikonal_coefficients, eikonal_loss, eikonal_loss_and_grad, eikonal_residual
    z = load(name)
    c = fixture_case(z)
    m = module(eval(str(z["kwargs"])))
    coef = eikonal_coefficients(c["tau"])
    assert coef["sq"] == c["sq"] and abs((0.5 * m.hx) * (0.5 * m.hy) - c["wscale"]) <= 1e-12
    u = cu(z["u"]).requires_grad_(True)
    loss = eikonal_loss(m, u, kind="norm", **coef)
    g, = torch.autograd.grad(loss, u)
    ref, pt = z["grad"], float(z["point_terms"])
    print(name, "loss rel", abs(float(loss.detach()) + pt - float(z["loss"])) / float(z["loss"]), "grad", float(np.abs(g.cpu().numpy() - ref).max() / np.abs(ref).max()))
    np.testing.assert_allclose(float(loss.detach()) + pt, float(z["loss"]), rtol=LOSS_RTOL)
    close(g, ref, rtol=GRAD_RTOL, arel=GRAD_AREL)
    l2, g2 = eikonal_loss_and_grad(m, u.detach(), kind="norm", **coef)
    assert l2.dtype == torch.float32 and l2.dim() == 0
    np.testing.assert_allclose(float(l2) + pt, float(z["loss"]), rtol=LOSS_RTOL)
    close(g2, ref, rtol=GRAD_RTOL, arel=GRAD_AREL)
    assert torch.equal(g2, g) and torch.equal(l2, loss.detach())
    close(eikonal_residual(m, u.detach(), **coef)[0, 0], z["R1"], rtol=GRAD_RTOL, arel=GRAD_AREL)


def _cases(shape, P, ngp):
    """(name, kwargs): every compile-time form (mask none / constants / value fields; forcing constant / nodal / Gauss points, shared and
    per sample) at least once; masks fp32 / uint8 / bool, shared and per sample, overlapping; tau = 0 and tau = 0.25"""
    B, _, ny, nx = shape
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(3)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float())
    shared = wall[:1].contiguous()
    G, eshape = ngp * ngp, ((ny - 1) // P, (nx - 1) // P)
    f_sh = cu(seeded((G, *eshape), 20, 0.5))
    f_b = cu(seeded((B, G, *eshape), 21, 0.5))
    fn_sh = cu(seeded((1, 1, ny, nx), 22, 0.5))
    fn_b = cu(seeded(shape, 23, 0.5))
    vfield = 0.3 * cu(seeded(shape, 30, -0.5))
    vshared = 0.3 * cu(seeded((1, 1, ny, nx), 31, -0.5))
    return [
        ("no masks, the scripts' constants", dict(tau=0.25)),
        ("no masks, nodal forcing shared, unstabilised", dict(f=fn_sh, tau=0.0, sq=1.0)),
        ("fp32 shared + per sample, constants, gp forcing per sample", dict(bc=(shared, blob), bc_values=(0.1, 0.0), f_gp=f_b, tau=0.25)),
        ("fp32 overlapping, value fields, gp forcing shared", dict(bc=(wall, blob), bc_values=(vfield, vshared), f_gp=f_sh, tau=0.25, sq=0.9)),
        ("u8 per sample + bool shared, value field + constant, nodal forcing per sample", dict(bc=(blob.to(torch.uint8), shared.bool()), bc_values=(vshared, 0.05), f=fn_b, tau=0.25)),
        ("bool only condition 2, constant forcing, tau 0", dict(bc=(None, blob.bool()), bc_values=(0.0, -0.1), f_gp=0.7, tau=0.0)),
        ("u8 shared, value field per sample, the scripts' constants", dict(bc=(shared.to(torch.uint8), None), bc_values=(vfield, 0.0), tau=0.25)),
    ]


@pytest.mark.parametrize("P,ngp,nelx,nely,B", SHAPES)
def test_eikonal_fused_matches_composed(P, ngp, nelx, nely, B):
    from diffnet_amd import eikonal as ek
    m = hh_module(P, ngp, nelx, nely)
    shape = (B, 1, P * nely + 1, P * nelx + 1)
    u = field(shape, 10)
    cot = cu(seeded(shape, 11, -0.5))
    for name, kw in _cases(shape, P, ngp):
        fixed = _fixed(kw.get("bc"), shape)
        R, Rc = ek.eikonal_residual(m, u, **kw), ek.eikonal_residual_composed(m, u, **kw)
        dr = _max_rel(R, Rc)
        assert dr <= RTOL_R, (name, "R", dr)
        assert float(R[fixed].abs().max() if fixed.any() else 0.0) == 0.0, name
        dist = [dr]
        for kind in ("norm", "sumsq"):
            ua, ub = u.clone().requires_grad_(True), u.clone().requires_grad_(True)
            la = ek.eikonal_loss(m, ua, kind=kind, **kw)
            rc = ek.eikonal_residual_composed(m, ub, **kw)
            lb = torch.norm(rc) if kind == "norm" else torch.sum(rc ** 2)
            ga, = torch.autograd.grad(la, ua)
            gb, = torch.autograd.grad(lb, ub)
            l2, g2 = ek.eikonal_loss_and_grad(m, u, kind=kind, **kw)
            la, lb = float(la.detach()), float(lb.detach())      # both are 0 where every node is a Dirichlet node (the 2 x 2 mesh with the wall)
            dl, dg = abs(la - lb) / max(abs(lb), 1e-30), _max_rel(ga, gb)
            dist += [dl, dg]
            assert abs(la - lb) <= RTOL_LOSS * abs(lb) and abs(float(l2) - lb) <= RTOL_LOSS * abs(lb), (name, kind, "loss", dl)
            assert dg <= RTOL_G, (name, kind, "gradient", dg)
            assert torch.equal(g2, ga), (name, kind)
            assert float(ga[fixed].abs().max() if fixed.any() else 0.0) == 0.0, (name, kind)
        # the VJP launch with a cotangent that is not R
        ua, ub = u.clone().requires_grad_(True), u.clone().requires_grad_(True)
        ga, = torch.autograd.grad((ek.eikonal_residual(m, ua, **kw) * cot).sum(), ua)
        gb, = torch.autograd.grad((ek.eikonal_residual_composed(m, ub, **kw) * cot).sum(), ub)
        dv = _max_rel(ga, gb)
        print((P, ngp, nelx, nely, B), name, "R", dist[0], "| norm: loss", dist[1], "grad", dist[2], "| sumsq: loss", dist[3], "grad", dist[4], "| vjp", dv)
        assert dv <= RTOL_G, (name, "vjp", dv)
        assert float(ga[fixed].abs().max() if fixed.any() else 0.0) == 0.0, name


def test_eikonal_dirichlet_nodes_and_condition_order():
    from diffnet_amd import eikonal as ek
    P, ngp, nelx, nely, B = 2, 3, 70, 9, 3
    m = hh_module(P, ngp, nelx, nely)
    shape = (B, 1, P * nely + 1, P * nelx + 1)
    u = field(shape, 90)
    m1 = torch.zeros(shape)
    m1[..., 0, :] = 1.0
    m2 = torch.zeros(shape)
    m2[..., :, 0] = 1.0
    m2[..., :, -1] = 1.0
    m1, m2 = m1.to(dev()), m2.to(dev())
    kw = dict(bc=(m1, m2), bc_values=(0.3 * cu(seeded(shape, 93, 0.5)), -0.2), tau=0.25)
    fixed = (m1 > 0.5) | (m2 > 0.5)
    R = ek.eikonal_residual(m, u, **kw)
    loss, g = ek.eikonal_loss_and_grad(m, u, **kw)
    assert float(R[fixed].abs().max()) == 0.0 and float(R[~fixed].abs().max()) > 0
    assert float(g[fixed].abs().max()) == 0.0 and float(g[~fixed].abs().max()) > 0
    np.testing.assert_allclose(float(loss), float(torch.norm(R.double())), rtol=1e-6)
    # where both masks hold condition 2's value is the one used
    both = (m1 > 0.5) & (m2 > 0.5)
    l_a, g_a = ek.eikonal_loss_and_grad(m, u, **dict(kw, bc=(m1 * (~both).float(), m2)))
    assert torch.equal(l_a, loss) and torch.equal(g_a, g)
    l_b, _ = ek.eikonal_loss_and_grad(m, u, **dict(kw, bc=(m1, m2 * (~both).float())))
    assert not torch.equal(l_b, loss)
    # a backward with a scaled grad_output; a loss of a field without gradient computes none
    ur = u.clone().requires_grad_(True)
    ga, = torch.autograd.grad(3.0 * ek.eikonal_loss(m, ur, **kw), ur)
    assert _max_rel(ga, 3.0 * g) <= 1e-6
    assert not ek.eikonal_loss(m, u, **kw).requires_grad


def test_eikonal_bitwise_across_batch_sizes_plans_and_runs():
    from diffnet_amd import _lib, ops
    P, ngp, nelx, nely, B = 2, 3, 300, 37, 3          # Q = 301 thread columns: five one-wave chunks by default
    m = hh_module(P, ngp, nelx, nely)
    shape = (B, 1, P * nely + 1, P * nelx + 1)
    u = field(shape, 70)
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(9)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float()).to(torch.uint8)
    vals = (0.3 * cu(seeded(shape, 80, -0.5)), 0.1)
    f = cu(seeded((B, ngp * ngp, nely, nelx), 81, 0.5))
    cot = cu(seeded(shape, 82, -0.5))
    kw = dict(tau=0.25, wscale=0.7)

    def fwd(uu=u, bc=(wall, blob), vv=vals, ff=f, **over):
        return ops.eikonal_apply(m.geom, uu, bc, vv, None, ff, **{**kw, **dict(want_sumsq=True, want_norm=True), **over})

    def vjp(uu=u, bc=(wall, blob), vv=vals, cc=cot):
        return ops.eikonal_apply(m.geom, uu, bc, vv, cot=cc, **kw)[0]

    o, s, nr = fwd()
    g = vjp()
    o2, s2, n2 = fwd()
    assert torch.equal(o, o2) and torch.equal(s, s2) and torch.equal(nr, n2) and torch.equal(g, vjp())       # run to run
    o3, s3, n3 = fwd(want_sumsq=False, want_norm=False)
    assert s3 is None and n3 is None and torch.equal(o3, o)
    o4, s4, n4 = fwd(want_out=False)
    assert o4 is None and torch.equal(s4, s) and torch.equal(n4, nr)
    np.testing.assert_allclose(float(s), float((o.double() ** 2).sum()), rtol=1e-6)
    np.testing.assert_allclose(float(nr), float(s) ** 0.5, rtol=1e-6)
    # sample k of the batch launched alone: the same bits
    for k in range(B):
        one = lambda t: t[k:k + 1].contiguous()                                 # noqa: E731
        ok, _, _ = fwd(one(u), (one(wall), one(blob)), (one(vals[0]), 0.1), one(f), want_sumsq=False, want_norm=False)
        assert torch.equal(o[k:k + 1], ok), k
        assert torch.equal(g[k:k + 1], vjp(one(u), (one(wall), one(blob)), (one(vals[0]), 0.1), one(cot))), k
    # other launch plans (threads per workgroup, element rows per strip; two chunks of three and of four waves): the same bits
    try:
        for plan in ("64,1", "192,3", "256,64"):
            _lib.config_set("PLAN_FSDT", plan)
            op, sp, _ = fwd()
            assert torch.equal(op, o) and torch.equal(vjp(), g), plan
            np.testing.assert_allclose(float(sp), float(s), rtol=1e-12)
            assert torch.equal(fwd()[1], sp), plan                                # the sum: bitwise for a given mesh, batch and plan
    finally:
        _lib.config_set("PLAN_FSDT", "")
    o5, s5, n5 = fwd()
    assert torch.equal(o5, o) and torch.equal(s5, s) and torch.equal(n5, nr)


def test_eikonal_workspace_is_isolated_from_a_helmholtz_launch():
    """Eikonal and Helmholtz launches interleaved on one stream, repeatedly: every result equals its stand-alone value bitwise (the
    reduction workspaces are separate) and the workspace status is clean afterwards."""
    import ctypes as C
    from diffnet_amd import _lib, ops
    from diffnet_amd.eikonal import eikonal_loss_and_grad
    m = hh_module(2, 3, 93, 24)
    shape = (2, 1, 49, 187)
    u = field(shape, 120)
    wall = boundary_mask(shape).to(dev())

    def ek():
        return eikonal_loss_and_grad(m, u, bc=(wall, None), bc_values=(0.1, 0.0), tau=0.25)

    def es():
        return ops.eikonal_apply(m.geom, u, (wall, None), (0.1, 0.0), tau=0.25, want_sumsq=True, want_norm=True)

    def hh():
        return ops.helmholtz_apply(m.geom, u, None, 9.0, (wall, None), (1.0, 0.0), None, 0.3, want_sumsq=True)

    refs = dict(e=ek(), s=es(), h=hh())
    seq = []
    for _ in range(3):
        seq += [("e", ek()), ("h", hh()), ("s", es()), ("h", hh())]
    seq += [("e", ek()), ("e", ek()), ("h", hh()), ("s", es())]
    torch.cuda.synchronize()
    for k, r in seq:
        for a, b in zip(r, refs[k]):
            assert torch.equal(a, b), k
    ops.workspace_status()
    assert ops._EIKONAL.ws and all(w is not v for w in ops._EIKONAL.ws.values() for v in ops._HELMHOLTZ.ws.values())
    for (_, stream), ws in ops._EIKONAL.ws.items():
        assert _lib.lib().dn_workspace_status(C.c_void_p(ws.data_ptr()), C.c_void_p(stream)) == 0


def test_eikonal_graph_capture_replays_bitwise():
    from diffnet_amd.eikonal import eikonal_loss_and_grad
    P, ngp, nelx, nely = 3, 4, 43, 15
    m = hh_module(P, ngp, nelx, nely)
    shape = (2, 1, P * nely + 1, P * nelx + 1)
    u = field(shape, 130)
    wall = boundary_mask(shape).to(dev())
    kw = dict(bc=(wall, wall[:1].to(torch.uint8)), bc_values=(0.3 * cu(seeded((1, 1, *shape[2:]), 134, -0.5)), 0.0), f=cu(seeded(shape, 135, 0.5)),
              tau=0.25)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):                     # warm-up on the capture stream: workspace, prepared call
            eager = eikonal_loss_and_grad(m, u, **kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):    # a single chain, no parallel branches
            static = eikonal_loss_and_grad(m, u, **kw)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static[0], eager[0]) and torch.equal(static[1], eager[1])


def test_eikonal_gradient_routing_no_silent_zero_gradients():
    from diffnet_amd import eikonal as ek
    from diffnet_amd._lib import DiffNetHipError
    m = module(dict(domain_size=17, fem_basis_deg=2))
    shape = (1, 1, 17, 17)
    u = field(shape, 1, (1.0, 1.0))
    wall = boundary_mask(shape).to(dev())
    mk = lambda seed, lo: cu(seeded(shape, seed, lo)).requires_grad_(True)      # noqa: E731
    f, v1 = mk(2, 0.5), mk(4, -0.5)
    fg = cu(seeded((9, 8, 8), 3, 0.5)).requires_grad_(True)
    for kw, wrt in ((dict(bc=(wall, None), bc_values=(v1, 0.0), f=f, tau=0.25), (v1, f)), (dict(f_gp=fg, tau=0.25), (fg,))):
        for kind in ("norm", "sumsq"):
            ua, ub = u.clone().requires_grad_(True), u.clone().requires_grad_(True)
            rc = ek.eikonal_residual_composed(m, ub, **kw)
            ga = torch.autograd.grad(ek.eikonal_loss(m, ua, kind=kind, **kw), (ua, *wrt))
            gb = torch.autograd.grad(torch.norm(rc) if kind == "norm" else torch.sum(rc ** 2), (ub, *wrt))
            for a, b in zip(ga, gb):
                assert a is not None and float(a.abs().max()) > 0 and _max_rel(a, b) <= RTOL_G
        ga = torch.autograd.grad(ek.eikonal_residual(m, u, **kw).sum(), wrt)
        assert all(a is not None and float(a.abs().max()) > 0 for a in ga)
    with pytest.raises(DiffNetHipError):
        ek.eikonal_loss(m, u, bc=(boundary_mask(shape), None))           # a CPU mask
    with pytest.raises(ValueError):
        ek.eikonal_loss(m, u, bc=(None, None), bc_values=(cu(seeded(shape, 7)), 0.0))     # a value field without its mask
    with pytest.raises(ValueError):
        ek.eikonal_loss(m, u, f=cu(seeded(shape, 8)), f_gp=cu(seeded((9, 8, 8), 9)))       # two forcings


def test_eikonal_example_fused_and_composed_agree():
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("ex_eikonal_2d", os.path.join(here, "..", "examples", "eikonal_2d.py"))
    ex = importlib.util.module_from_spec(spec)
    sys.modules["ex_eikonal_2d"] = ex
    spec.loader.exec_module(ex)
    for opt, steps in (("lbfgs", 4),):
        _, hf = ex.run(n=33, steps=steps, optimizer=opt, mode="fused", verbose=False)
        _, hc = ex.run(n=33, steps=steps, optimizer=opt, mode="composed", verbose=False)
        print(opt, "fused", hf, "composed", hc)
        assert hf[-1] < hf[0] and hc[-1] < hc[0], opt
        assert abs(hf[0] - hc[0]) <= 1e-4 * abs(hc[0]) and abs(hf[-1] - hc[-1]) <= 1e-4 * abs(hc[-1]), opt
