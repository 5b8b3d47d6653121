"""GPU tests of the fused 2-D strong-form least-squares loss (dn_strongform_apply, csrc/strongform.hip; diffnet_amd/strongform.py): against
the reference fixtures (tests/golden/loss_strongform_*.npz, the reference scripts' own `loss` bodies), against the same loss composed from
the drop-in operators on every compile-time form, degree and rule, on ragged meshes around the kernel's seams, the Dirichlet nodes,
bitwise independence of batch, launch plan and run, the sum against the composed Gauss-point residuals in fp64, isolation of its reduction
workspace from the other operators' launches, graph capture, gradient routing, the example and the scripts' own sizes."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import boundary_mask, close, cu, dev, load, module, seeded
from test_strongform_host import FIXTURE_TOL, FIXTURES, fixture_case, strongform_np

pytestmark = pytest.mark.gpu

BURGERS = (0.0, 1.0, 1.0, 0.0, 0.0, 0.0)
VISCOUS = (0.0, 1.0, 1.0, -0.01 / np.pi, 0.0, 0.0)
POISSON = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
LINEAR = (0.7, -0.4, 0.0, 0.0, 0.0, 0.9)
FULL = (0.3, 1.0, 1.2, -0.05, 0.02, 1.0)
# (degree, ngp, nelx, nely, B): nelx around C = 63, the element columns of a one-wave chunk (1, 2, C - 1, C, C + 1, 2C + 1, and 300:
# two chunks of the widest workgroup), nely around R = 4, the shortest strip (1, R - 1, R, R + 1, 3R + 2); nodes = degree * nel + 1
SHAPES = [(1, 2, 1, 1, 1), (1, 3, 2, 3, 3), (2, 3, 62, 4, 1), (2, 4, 63, 5, 3), (3, 3, 64, 14, 1), (3, 4, 127, 3, 3), (1, 4, 63, 14, 3),
          (2, 3, 300, 5, 1), (3, 4, 2, 1, 1)]


def sf_module(P, ngp, nelx, nely, lengths=(1.0, 0.7)):
    nx, ny = P * nelx + 1, P * nely + 1
    return module(dict(domain_sizes=(nx, ny), domain_lengths=lengths, domain_size=nx, domain_length=lengths[0], fem_basis_deg=P, ngp_1d=ngp))


def _max_rel(a, b):
    scale = max(float(b.abs().max()), float(a.abs().max()), 1e-30)
    return float((a - b).abs().max()) / scale


def _fixed(bc, shape):
    out = torch.zeros(shape, dtype=torch.bool, device=dev())
    for mk in (() if bc is None else bc):
        if mk is not None:
            out |= ((mk > 0.5) if mk.dtype == torch.float32 else (mk != 0)).expand(shape)
    return out


def fixture_inputs(z):
    c = fixture_case(z)
    m = module(eval(str(z["kwargs"])))
    v1 = c["vals"][0]
    v1 = cu(np.asarray(v1, dtype=np.float32)).reshape(1, 1, *z["u"].shape[-2:]) if np.ndim(v1) else float(v1)
    kw = dict(bc=(cu(z["mask1"]), cu(z["mask2"])), bc_values=(v1, 0.0), f=cu(z["forcing"]), coef=c["coef"], wscale=c["wscale"])
    return m, kw


@pytest.mark.parametrize("name", FIXTURES)
def test_strongform_vs_reference_golden(name):
    from diffnet_amd.strongform import strong_form_loss, strong_form_loss_and_grad
    z = load(name)
    m, kw = fixture_inputs(z)
    lrt, grt, gar = FIXTURE_TOL[name]
    u = cu(z["u"]).requires_grad_(True)
    loss = strong_form_loss(m, u, **kw)
    loss.backward()
    ref = z["grad"]
    print(name, "loss rel", abs(float(loss) - float(z["loss"])) / float(z["loss"]), "grad", float(np.abs(u.grad.cpu().numpy() - ref).max() / np.abs(ref).max()))
    np.testing.assert_allclose(float(loss), float(z["loss"]), rtol=lrt)
    close(u.grad, ref, rtol=grt, arel=gar)
    l2, g2 = strong_form_loss_and_grad(m, u.detach(), **kw)
    assert l2.dtype == torch.float64 and l2.dim() == 0
    np.testing.assert_allclose(float(l2), float(z["loss"]), rtol=lrt)
    close(g2, ref, rtol=grt, arel=gar)
    assert torch.equal(g2, u.grad)


def _cases(shape, P, ngp):
    """(name, bc, bc_values, f, f_gp, coef): every compile-time form (mask none / constants / value fields; forcing constant / nodal /
    Gauss points, shared and per sample; b = 0 and b != 0; second-order terms on and off) at least once; masks fp32 / uint8 / bool,
    shared and per sample"""
    B, _, ny, nx = shape
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(3)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float())
    shared = wall[:1].contiguous()
    G, eshape = ngp * ngp, ((ny - 1) // P, (nx - 1) // P)
    f_sh = cu(seeded((G, *eshape), 20, -0.5)) * 4.0
    f_b = cu(seeded((B, G, *eshape), 21, -0.5)) * 4.0
    fn_sh = cu(seeded((1, 1, ny, nx), 22, -0.5)) * 4.0
    fn_b = cu(seeded(shape, 23, -0.5)) * 4.0
    vfield = cu(seeded(shape, 30, -0.5))
    vshared = cu(seeded((1, 1, ny, nx), 31, -0.5))
    return [
        ("no masks, constant forcing, linear first order", None, (0.0, 0.0), None, 0.6, LINEAR),
        ("no masks, nodal forcing shared, all terms", None, (0.0, 0.0), fn_sh, None, FULL),
        ("fp32 shared + per sample, constants, gp forcing per sample, Burgers", (shared, blob), (1.0, 0.0), None, f_b, BURGERS[:5] + (0.5,)),
        ("fp32 overlapping, value fields, gp forcing shared, Poisson", (wall, blob), (vfield, vshared), None, f_sh, POISSON),
        ("u8 per sample + bool shared, value field + constant, nodal forcing per sample, Poisson", (blob.to(torch.uint8), shared.bool()),
         (vshared, 0.25), fn_b, None, POISSON),
        ("bool only condition 2, constant forcing, viscous Burgers", (None, blob.bool()), (0.0, -0.4), None, -1.3, VISCOUS[:5] + (1.0,)),
        ("u8 shared, value field per sample, gp forcing per sample, all terms", (shared.to(torch.uint8), None), (vfield, 0.0), None, f_b, FULL),
    ]


def _np64(t, b):
    if t is None or not isinstance(t, torch.Tensor):
        return t
    t = t[b if t.shape[0] > 1 else 0] if t.dim() == 4 else t
    return t.double().cpu().numpy()


def _float64(m, P, ngp, u, bc, vals, f, f_gp, coef, out_scale):
    """(sum, grad) of the float64 restatement (tests/test_strongform_host.py), sample by sample"""
    B = u.shape[0]
    tot, grads = 0.0, []
    for b in range(B):
        masks = [None if mk is None else (_np64(mk, b)[0] > 0.5) for mk in ((None, None) if bc is None else bc)]
        vv = [v if not isinstance(v, torch.Tensor) else _np64(v, b)[0] for v in vals]
        fg = f_gp if not isinstance(f_gp, torch.Tensor) else (_np64(f_gp, b) if f_gp.dim() == 4 else f_gp.double().cpu().numpy())
        s, g, _ = strongform_np(_np64(u, b)[0], masks, vv, coef, m.hx, m.hy, P, ngp, f=None if f is None else _np64(f, b)[0], f_gp=fg,
                                out_scale=out_scale)
        tot += s
        grads.append(g)
    return tot, torch.from_numpy(np.stack(grads)[:, None])


# Tolerances: gradient within 1e-4 of its largest entry, loss rtol 2e-5 -- the project's figures for fused against composed (transport,
# Navier-Stokes).  Where the composed route ITSELF is farther than that from the float64 restatement (fp32 sums of (2/h)^2-sized second
# derivatives), the fused route is bounded by 4 x the composed route's distance to float64 for that case instead.
@pytest.mark.parametrize("P,ngp,nelx,nely,B", SHAPES)
def test_strongform_fused_matches_composed(P, ngp, nelx, nely, B):
    from diffnet_amd.strongform import strong_form_loss, strong_form_loss_and_grad, strong_form_loss_composed
    m = sf_module(P, ngp, nelx, nely)
    shape = (B, 1, P * nely + 1, P * nelx + 1)
    u = cu(seeded(shape, 10, -0.5)) * 2.0
    for name, bc, vals, f, f_gp, coef in _cases(shape, P, ngp):
        kw = dict(bc=bc, bc_values=vals, f=f, f_gp=f_gp, coef=coef)
        ua, ub = u.clone().requires_grad_(True), u.clone().requires_grad_(True)
        la, lb = strong_form_loss(m, ua, **kw), strong_form_loss_composed(m, ub, **kw)
        ga, = torch.autograd.grad(la, ua)
        gb, = torch.autograd.grad(lb, ub)
        dl, dg = abs(float(la) - float(lb)) / max(abs(float(lb)), 1e-30), _max_rel(ga, gb)
        print((P, ngp, nelx, nely, B), name, "loss", dl, "grad", dg)
        ltol, gtol = 2e-5, 1e-4
        if dl > ltol or dg > gtol:
            s64, g64 = _float64(m, P, ngp, u, bc, vals, f, f_gp, coef, 1.0 / (B * nelx * nely))
            l64 = s64 / (B * nelx * nely)
            cl, cg = abs(float(lb) - l64) / abs(l64), _max_rel(gb.double().cpu(), g64)
            fl, fg = abs(float(la) - l64) / abs(l64), _max_rel(ga.double().cpu(), g64)
            print("    against float64: composed loss", cl, "grad", cg, "fused loss", fl, "grad", fg)
            if cl > ltol:
                ltol, dl = 4 * cl, fl
            if cg > gtol:
                gtol, dg = 4 * cg, fg
        assert dl <= ltol, (name, "loss", dl, ltol)
        assert dg <= gtol, (name, "gradient", dg, gtol)
        assert float(ga[_fixed(bc, shape)].abs().max() if _fixed(bc, shape).any() else 0.0) == 0.0, name
        l2, g2 = strong_form_loss_and_grad(m, u, reduction="sum", **kw)
        np.testing.assert_allclose(float(l2), float(la) * B * nelx * nely, rtol=1e-6, err_msg=name)


def test_strongform_dirichlet_nodes_and_overlap_rule():
    from diffnet_amd.strongform import strong_form_loss_and_grad
    P, ngp, nelx, nely = 2, 3, 20, 9
    m = sf_module(P, ngp, nelx, nely)
    shape = (2, 1, P * nely + 1, P * nelx + 1)
    u = cu(seeded(shape, 90, -0.5))
    m1 = torch.zeros(shape)
    m1[..., 0, :] = 1.0
    m2 = torch.zeros(shape)
    m2[..., :, 0] = 1.0
    m2[..., :, -1] = 1.0
    m1, m2 = m1.to(dev()), m2.to(dev())
    v1 = cu(seeded(shape, 91, 0.5))
    loss, g = strong_form_loss_and_grad(m, u, (m1, m2), (v1, -0.75), coef=FULL)
    fixed = (m1 > 0.5) | (m2 > 0.5)
    assert float(g[fixed].abs().max()) == 0.0 and float(g[~fixed].abs().max()) > 0
    # where both masks hold condition 2's value is the one used: the same numbers with the overlap removed from condition 1, other
    # numbers with the overlap removed from condition 2
    both = (m1 > 0.5) & (m2 > 0.5)
    l_a, g_a = strong_form_loss_and_grad(m, u, (m1 * (~both).float(), m2), (v1, -0.75), coef=FULL)
    assert torch.equal(l_a, loss) and torch.equal(g_a, g)
    l_b, _ = strong_form_loss_and_grad(m, u, (m1, m2 * (~both).float()), (v1, -0.75), coef=FULL)
    assert abs(float(l_b) - float(loss)) > 1e-4 * abs(float(loss))
    s64, g64 = _float64(m, P, ngp, u, (m1, m2), (v1, -0.75), None, None, FULL, 1.0 / (2 * nelx * nely))
    np.testing.assert_allclose(float(loss), s64 / (2 * nelx * nely), rtol=2e-5)
    assert _max_rel(g.double().cpu(), g64) <= 1e-4
    # the values under the masks do not matter
    u2 = torch.where(fixed, torch.full_like(u, 7.0), u)
    l_c, g_c = strong_form_loss_and_grad(m, u2, (m1, m2), (v1, -0.75), coef=FULL)
    assert torch.equal(l_c, loss) and torch.equal(g_c, g)


def test_strongform_bitwise_across_batch_sizes_plans_and_runs():
    from diffnet_amd import _lib, ops
    from diffnet_amd.strongform import strong_form_residual_composed
    P, ngp, nelx, nely, B = 2, 3, 130, 37, 3
    m = sf_module(P, ngp, nelx, nely)
    shape = (B, 1, P * nely + 1, P * nelx + 1)
    u = cu(seeded(shape, 70, -0.5))
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(9)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float()).to(torch.uint8)
    vals = (cu(seeded(shape, 80, -0.5)), 0.2)
    f = cu(seeded((B, ngp * ngp, nely, nelx), 81, -0.5))
    kw = dict(coef=FULL, wscale=0.7, out_scale=0.01)
    g, s = ops.strongform_apply(m.geom, u, (wall, blob), vals, None, f, **kw)
    g2, s2 = ops.strongform_apply(m.geom, u, (wall, blob), vals, None, f, **kw)
    assert torch.equal(g, g2) and torch.equal(s, s2)                             # run to run
    g_only, none = ops.strongform_apply(m.geom, u, (wall, blob), vals, None, f, want_sum=False, **kw)
    none2, s_only = ops.strongform_apply(m.geom, u, (wall, blob), vals, None, f, want_grad=False, **kw)
    assert none is None and none2 is None and torch.equal(g_only, g) and torch.equal(s_only, s)
    # the sum against the composed Gauss-point residuals, added in fp64
    r = strong_form_residual_composed(m, u, (wall, blob), vals, None, f, FULL)
    w = (m.gpw.to(dev()).double() * 0.7).reshape(1, -1, 1, 1)
    np.testing.assert_allclose(float(s), float((w * r.double() ** 2).sum()), rtol=1e-6)
    # sample k of the batch launched alone: the same bits
    for k in range(B):
        one = lambda t: t[k:k + 1].contiguous()                                 # noqa: E731
        gk, _ = ops.strongform_apply(m.geom, one(u), (one(wall), one(blob)), (one(vals[0]), 0.2), None, one(f), want_sum=False, **kw)
        assert torch.equal(g[k:k + 1], gk), k
    # other launch plans (threads per workgroup, element rows per strip): the same bits
    try:
        for plan in ("64,1", "64,5", "192,3", "256,64"):
            _lib.config_set("PLAN_FSDT", plan)
            gp, sp = ops.strongform_apply(m.geom, u, (wall, blob), vals, None, f, **kw)
            assert torch.equal(gp, g), plan
            np.testing.assert_allclose(float(sp), float(s), rtol=1e-12)
    finally:
        _lib.config_set("PLAN_FSDT", "")
    g3, s3 = ops.strongform_apply(m.geom, u, (wall, blob), vals, None, f, **kw)
    assert torch.equal(g3, g) and torch.equal(s3, s)


def test_strongform_chained_between_transport_and_poisson_on_one_stream():
    """One strong-form launch between a transport launch and a Poisson launch, repeatedly: nobody's sums or outputs change (the three
    reduction workspaces are separate)."""
    from diffnet_amd import ops
    m = sf_module(2, 3, 93, 64)
    shape = (2, 1, 129, 187)
    u = cu(seeded(shape, 120, -0.5))
    wall = boundary_mask(shape).to(dev())
    tm = module(dict(domain_size=129))
    tshape = (2, 1, 129, 129)
    tu, tnu, tf = (cu(seeded(tshape, 121 + i, 0.5 if i == 1 else -0.5)) for i in range(3))
    twall = boundary_mask(tshape).to(dev())

    def sf():
        return ops.strongform_apply(m.geom, u, (wall, None), (1.0, 0.0), None, 0.3, coef=FULL)

    def tr():
        out, sums, norm = ops.transport_apply(tm.geom, tu, None, (twall, None), (1.0, 0.0), f_gp=0.3, want_norm=True, adv=(0.0, 1.0), kappa=(0.04, 0.04),
                                              react=(-8.0, 32.0, -96.0, 64.0))
        return out, sums, norm

    def po():
        return tm.energy_loss_and_grad(tu, tnu, tf, dirichlet=[(twall, 0.0)])

    refs = dict(s=sf(), t=tr(), p=po())
    seq = []
    for _ in range(3):
        seq += [("t", tr()), ("s", sf()), ("p", po())]
    seq += [("s", sf()), ("s", sf()), ("p", po()), ("s", sf()), ("t", tr())]
    torch.cuda.synchronize()
    for k, r in seq:
        for a, b in zip(r, refs[k]):
            assert torch.equal(a, b), k


def test_strongform_loss_and_grad_graph_capture_replays_bitwise():
    from diffnet_amd.strongform import strong_form_loss_and_grad
    P, ngp, nelx, nely = 3, 4, 43, 15
    m = sf_module(P, ngp, nelx, nely)
    shape = (2, 1, P * nely + 1, P * nelx + 1)
    u = cu(seeded(shape, 130, -0.5))
    wall = boundary_mask(shape).to(dev())
    kw = dict(bc=(wall, wall[:1].to(torch.uint8)), bc_values=(cu(seeded((1, 1, *shape[2:]), 134, -0.5)), 0.0), f=cu(seeded(shape, 135, -0.5)), coef=FULL)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):                     # warm-up on the capture stream: workspace, prepared call
            eager = strong_form_loss_and_grad(m, u, **kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            static = strong_form_loss_and_grad(m, u, **kw)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static[0], eager[0]) and torch.equal(static[1], eager[1])
    with torch.no_grad():
        u.mul_(0.5)                            # replays read the field in place
    g.replay()
    again = strong_form_loss_and_grad(m, u, **kw)
    torch.cuda.synchronize()
    assert torch.equal(static[0], again[0]) and torch.equal(static[1], again[1]) and not torch.equal(static[0], eager[0])


def test_strongform_no_silent_zero_gradients_and_errors():
    from diffnet_amd import ops
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd.strongform import strong_form_loss, strong_form_loss_and_grad
    m = module(dict(domain_size=17, fem_basis_deg=2))
    shape = (1, 1, 17, 17)
    u = cu(seeded(shape, 1, -0.5))
    wall = boundary_mask(shape).to(dev())
    f = cu(seeded(shape, 2, -0.5)).requires_grad_(True)
    fg = cu(seeded((9, 8, 8), 3, -0.5)).requires_grad_(True)
    v1 = cu(seeded(shape, 4, -0.5)).requires_grad_(True)
    ur = u.clone().requires_grad_(True)
    loss = strong_form_loss(m, ur, (wall, None), (v1, 0.0), f=f, coef=FULL)
    gs = torch.autograd.grad(loss, (ur, f, v1))
    assert all(float(g.abs().max()) > 0 for g in gs)
    loss = strong_form_loss(m, ur, (wall, None), (0.5, 0.0), f_gp=fg, coef=FULL)
    gs = torch.autograd.grad(loss, (ur, fg))
    assert all(float(g.abs().max()) > 0 for g in gs)
    # the fused route and the composed one are the same function of u
    l_f = strong_form_loss(m, ur, (wall, None), (v1.detach(), 0.0), f=f.detach(), coef=FULL)
    l_c = strong_form_loss(m, ur, (wall, None), (v1, 0.0), f=f, coef=FULL)
    np.testing.assert_allclose(float(l_f), float(l_c), rtol=2e-5)
    # a backward with a scaled grad_output scales the saved gradient; a loss of a field without gradient computes none
    ga, = torch.autograd.grad(3.0 * strong_form_loss(m, ur, coef=BURGERS), ur)
    _, gb = strong_form_loss_and_grad(m, u, coef=BURGERS)
    assert torch.equal(ga, 3.0 * gb)
    assert not strong_form_loss(m, u, coef=BURGERS).requires_grad
    with pytest.raises(ValueError):
        strong_form_loss(m, u, coef=BURGERS, reduction="max")
    with pytest.raises(ValueError):
        strong_form_loss_and_grad(m, u, coef=BURGERS, reduction="none")
    m_bad = module(dict(domain_sizes=(17, 16), domain_lengths=(1.0, 1.0), domain_size=17, domain_length=1.0, fem_basis_deg=2))
    with pytest.raises(ValueError):
        strong_form_loss(m_bad, cu(seeded((1, 1, 16, 17), 5, -0.5)), coef=BURGERS)
    with pytest.raises(DiffNetHipError):
        strong_form_loss(m, u, (boundary_mask(shape), None), coef=BURGERS)             # a CPU mask
    with pytest.raises(ValueError):
        ops.strongform_apply(m.geom, u, (None, None), (v1.detach(), 0.0), coef=BURGERS)     # a value field without its mask
    with pytest.raises(ValueError):
        ops.strongform_apply(m.geom, u, f=f.detach(), f_gp=fg.detach(), coef=POISSON)       # two forcings


def test_strongform_example_fused_and_composed_agree():
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("ex_burgers_space_time", os.path.join(here, "..", "examples", "burgers_space_time.py"))
    ex = importlib.util.module_from_spec(spec)
    sys.modules["ex_burgers_space_time"] = ex
    spec.loader.exec_module(ex)
    _, hf = ex.run(n=33, steps=5, optimizer="adam", verbose=False, mode="fused")
    _, hc = ex.run(n=33, steps=5, optimizer="adam", verbose=False, mode="composed")
    np.testing.assert_allclose(np.array(hf), np.array(hc), rtol=1e-3)
    assert hf[-1] < hf[0]


@pytest.mark.parametrize("P,n,coef", [(2, 257, BURGERS), (3, 256, POISSON)], ids=["burgers-257-q2", "poisson-256-q3"])
def test_strongform_full_size_properties(P, n, coef):
    """The scripts' own sizes at B = 1 (no oracle at that size): finite values, zero gradient on the Dirichlet nodes, the sum against the
    fp64 sum of the composed route's Gauss-point residuals."""
    from diffnet_amd.strongform import strong_form_loss_and_grad, strong_form_residual_composed
    m = module(dict(domain_size=n, fem_basis_deg=P))
    shape = (1, 1, n, n)
    u = cu(seeded(shape, 140, -0.5)) * 2.0
    wall = boundary_mask(shape).to(dev())
    f = cu(seeded(shape, 141, -0.5))
    kw = dict(bc=(None, wall), bc_values=(0.0, 0.0), f=f, coef=coef)
    loss, g = strong_form_loss_and_grad(m, u, reduction="sum", **kw)
    assert torch.isfinite(loss) and torch.isfinite(g).all() and float(g.abs().max()) > 0
    assert float(g[wall > 0.5].abs().max()) == 0.0
    r = strong_form_residual_composed(m, u, **kw)
    ref = float((m.gpw.to(dev()).double().reshape(1, -1, 1, 1) * r.double() ** 2).sum())
    np.testing.assert_allclose(float(loss), ref, rtol=1e-6)
