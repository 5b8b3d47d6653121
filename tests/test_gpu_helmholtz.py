"""GPU tests of the fused 2-D Helmholtz energy and weak-form residual (dn_helmholtz_apply, csrc/helmholtz.hip; diffnet_amd/helmholtz.py):
against the reference fixtures (tests/golden/loss_helmholtz_*.npz, the reference scripts' own `loss` bodies), against the same functions
composed from the drop-in operators and against the float64 restatement of tests/test_helmholtz_host.py on every compile-time form,
degree and rule, on ragged meshes around the kernel's seams; the residual route, the Dirichlet nodes, bitwise independence of batch,
launch plan and run, isolation of its reduction workspace from the other operators' launches, graph capture, gradient routing, the
example and the scripts' own size."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import boundary_mask, close, cu, dev, load, module, seeded
from test_helmholtz_host import FIXTURE_TOL, FIXTURES, fixture_case, helmholtz_np

pytestmark = pytest.mark.gpu

# (degree, ngp, nelx, nely, B): nelx around C = 63, the element columns of a one-wave chunk (1, 2, C - 1, C, C + 1, 2C + 1), and 510:
# Q = 511 thread columns, which the plan serves with two chunks of the widest workgroup (T = 256 scores 511 / 512 + 0.077 against at
# most 0.95 for 64, 128 and 192 threads), so the column recomputed across a chunk seam lies inside a four-wave workgroup; nely around
# R = 4, the shortest strip (1, R - 1, R, R + 1, 3R + 2); nodes = degree * nel + 1.  Every (degree, rule) pair of the domain once.  The
# plan test below runs 300 element columns as five one-wave chunks (the default), two chunks of 192 and two of 256 threads.
SHAPES = [(1, 2, 1, 1, 1), (1, 3, 2, 3, 3), (2, 3, 62, 4, 1), (2, 4, 63, 5, 3), (3, 3, 64, 14, 1), (3, 4, 127, 3, 3), (1, 4, 63, 14, 3),
          (2, 3, 510, 5, 1), (3, 4, 2, 1, 1)]
LENGTHS = (1.0, 0.7)
# the project's fused-against-composed figures (tests/test_gpu_strongform.py): gradient within 1e-4 of its largest entry, energy within
# 2e-5 of the gross sum sum W (c nu |grad u|^2 + cr |sg| u^2 + |fs u f|)
ETOL, GTOL = 2e-5, 1e-4


def hh_module(P, ngp, nelx, nely, lengths=LENGTHS):
    nx, ny = P * nelx + 1, P * nely + 1
    return module(dict(domain_sizes=(nx, ny), domain_lengths=lengths, domain_size=nx, domain_length=lengths[0], fem_basis_deg=P, ngp_1d=ngp))


def smooth(shape, seed, lengths=LENGTHS):
    """0.5 sin(pi x / Lx) sin(pi y / Ly) + 0.05 * seeded noise, as in the fixtures: the three terms of the energy stay comparable"""
    B, _, ny, nx = shape
    sx, sy = torch.sin(torch.linspace(0, np.pi, nx)), torch.sin(torch.linspace(0, np.pi, ny))
    return cu(0.5 * sy[:, None] * sx[None, :] + 0.05 * (2.0 * seeded(shape, seed) - 1.0))


def _max_rel(a, b):
    scale = max(float(b.abs().max()), float(a.abs().max()), 1e-30)
    return float((a - b).abs().max()) / scale


def _fixed(bc, shape):
    out = torch.zeros(shape, dtype=torch.bool, device=dev())
    for mk in (() if bc is None else bc):
        if mk is not None:
            out |= ((mk > 0.5) if mk.dtype == torch.float32 else (mk != 0)).expand(shape)
    return out


def _np64(t, b):
    if t is None or not isinstance(t, torch.Tensor):
        return t
    t = t[b if t.shape[0] > 1 else 0] if t.dim() == 4 else t
    return t.double().cpu().numpy()


def _float64(m, P, ngp, u, kw, ecoef=(0.5, 0.5, 1.0), ocoef=None, out_scale=1.0):
    """dict(energy, out, sumsq, gross) of the float64 restatement (tests/test_helmholtz_host.py), sample by sample"""
    bc, vals = kw.get("bc"), kw.get("bc_values", (0.0, 0.0))
    nu, sigma, f, f_gp = kw.get("nu"), kw.get("sigma", 0.0), kw.get("f"), kw.get("f_gp")
    en = ss = gross = 0.0
    outs = []
    for b in range(u.shape[0]):
        masks = [None if mk is None else (_np64(mk, b)[0] > 0.5) for mk in ((None, None) if bc is None else bc)]
        vv = [v if not isinstance(v, torch.Tensor) else _np64(v, b)[0] for v in vals]
        fg = f_gp if not isinstance(f_gp, torch.Tensor) else (_np64(f_gp, b) if f_gp.dim() == 4 else f_gp.double().cpu().numpy())
        r = helmholtz_np(_np64(u, b)[0], masks, vv, m.hx, m.hy, P, ngp, nu=None if nu is None else _np64(nu, b)[0],
                         sigma=_np64(sigma, b)[0] if isinstance(sigma, torch.Tensor) else sigma, f=None if f is None else _np64(f, b)[0],
                         f_gp=fg, ecoef=ecoef, ocoef=ocoef, out_scale=out_scale)
        en, ss, gross = en + r["energy"], ss + r["sumsq"], gross + sum(r["gross"])
        outs.append(r["out"])
    return dict(energy=en, sumsq=ss, gross=gross, out=torch.from_numpy(np.stack(outs)[:, None]))


def fixture_inputs(z):
    c = fixture_case(z)
    m = module(eval(str(z["kwargs"])))
    kw = dict(nu=cu(z["inputs"][:, 0:1]), sigma=c["sigma"], bc=(cu(z["mask1"]), cu(z["mask2"])), bc_values=(1.0, 0.0), f=cu(z["forcing"]))
    return m, kw, c


@pytest.mark.parametrize("name", FIXTURES)
def test_helmholtz_vs_reference_golden(name):
    from diffnet_amd.helmholtz import helmholtz_energy_loss, helmholtz_energy_loss_and_grad
    z = load(name)
    m, kw, c = fixture_inputs(z)
    lrt, grt, gar = FIXTURE_TOL[name]
    gross = sum(helmholtz_np(z["u"][0, 0].astype(np.float64), **c)["gross"]) * c["out_scale"]
    u = cu(z["u"]).requires_grad_(True)
    loss = helmholtz_energy_loss(m, u, **kw)
    loss.backward()
    ref = z["grad"]
    print(name, "loss / gross", abs(float(loss.detach()) - float(z["loss"])) / gross, "grad", float(np.abs(u.grad.cpu().numpy() - ref).max() / np.abs(ref).max()))
    assert abs(float(loss.detach()) - float(z["loss"])) <= lrt * gross
    close(u.grad, ref, rtol=grt, arel=gar)
    l2, g2 = helmholtz_energy_loss_and_grad(m, u.detach(), **kw)
    assert l2.dtype == torch.float64 and l2.dim() == 0
    assert abs(float(l2) - float(z["loss"])) <= lrt * gross
    close(g2, ref, rtol=grt, arel=gar)
    assert torch.equal(g2, u.grad)


def _cases(shape, P, ngp):
    """(name, kwargs): every compile-time form (mask none / constants / value fields; forcing constant / nodal / Gauss points, shared and
    per sample; coefficients none / constant sigma / fields) at least once; masks fp32 / uint8 / bool, shared and per sample, overlapping;
    nu absent or a field; sigma 0, a constant, a field shared or per sample, and large enough to make the energy negative"""
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
    nu_b, nu_sh = cu(seeded(shape, 40, 0.5)), cu(seeded((1, 1, ny, nx), 41, 0.5))
    sg_b, sg_sh = cu(seeded(shape, 42, 0.0)) * 30.0, cu(seeded((1, 1, ny, nx), 43, -0.25)) * 8.0
    # above the largest eigenvalue of the discrete Laplacian (of the order P^4 / h^2 per axis): the quadratic part of the energy is negative
    big = 100.0 * P ** 4 * max(eshape[1] / LENGTHS[0], eshape[0] / LENGTHS[1]) ** 2
    return [
        ("no masks, constant forcing, no reaction", dict(f_gp=0.6)),
        ("no masks, nodal forcing shared, constant sigma", dict(f=fn_sh, sigma=3.0)),
        ("fp32 shared + per sample, constants, gp forcing per sample, nu per sample + sigma 0", dict(bc=(shared, blob), bc_values=(1.0, 0.0), f_gp=f_b, nu=nu_b)),
        ("fp32 overlapping, value fields, gp forcing shared, a large sigma: a negative energy", dict(bc=(wall, blob), bc_values=(vfield, vshared), f_gp=f_sh, sigma=big)),
        ("u8 per sample + bool shared, value field + constant, nodal forcing per sample, nu shared + sigma per sample",
         dict(bc=(blob.to(torch.uint8), shared.bool()), bc_values=(vshared, 0.25), f=fn_b, nu=nu_sh, sigma=sg_b)),
        ("bool only condition 2, constant forcing, sigma field shared", dict(bc=(None, blob.bool()), bc_values=(0.0, -0.4), f_gp=-1.3, sigma=sg_sh)),
        ("u8 shared, value field per sample, no forcing, nu per sample + constant sigma", dict(bc=(shared.to(torch.uint8), None), bc_values=(vfield, 0.0), nu=nu_b, sigma=64.0)),
    ]


@pytest.mark.parametrize("P,ngp,nelx,nely,B", SHAPES)
def test_helmholtz_fused_matches_composed_and_float64(P, ngp, nelx, nely, B):
    from diffnet_amd.helmholtz import helmholtz_energy_loss, helmholtz_energy_loss_and_grad, helmholtz_energy_loss_composed
    m = hh_module(P, ngp, nelx, nely)
    shape = (B, 1, P * nely + 1, P * nelx + 1)
    u = smooth(shape, 10)
    nel = B * nelx * nely
    negative = False
    for name, kw in _cases(shape, P, ngp):
        ua, ub = u.clone().requires_grad_(True), u.clone().requires_grad_(True)
        la, lb = helmholtz_energy_loss(m, ua, **kw), helmholtz_energy_loss_composed(m, ub, **kw)
        ga, = torch.autograd.grad(la, ua)
        gb, = torch.autograd.grad(lb, ub)
        r64 = _float64(m, P, ngp, u, kw, out_scale=1.0 / nel)
        l64, gross, g64 = r64["energy"] / nel, r64["gross"] / nel, r64["out"]
        l2, g2 = helmholtz_energy_loss_and_grad(m, u, reduction="sum", **kw)
        negative = negative or ("negative" in name and l64 < 0)
        la, lb = la.detach(), lb.detach()
        dl, dg = abs(float(la) - float(lb)) / gross, _max_rel(ga, gb)
        cl, cg = abs(float(lb) - l64) / gross, _max_rel(gb.double().cpu(), g64)
        fl, fg = abs(float(l2) / nel - l64) / gross, _max_rel(ga.double().cpu(), g64)
        print((P, ngp, nelx, nely, B), name, "fused-composed: loss", dl, "grad", dg, "| composed-f64:", cl, cg, "| fused-f64:", fl, fg)
        etol, gtol = max(ETOL, 4 * cl), max(GTOL, 4 * cg)      # where the composed route itself is farther from float64: 4 x its distance
        assert dl <= etol and fl <= etol, (name, "energy", dl, fl, etol)
        assert dg <= gtol and fg <= gtol, (name, "gradient", dg, fg, gtol)
        fixed = _fixed(kw.get("bc"), shape)
        assert float(ga[fixed].abs().max() if fixed.any() else 0.0) == 0.0, name
        assert abs(float(l2) / nel - float(la)) <= 1e-6 * gross, name            # the same fp64 sum, rounded to fp32 by the autograd route
    assert negative                                  # the case with the large sigma


def test_helmholtz_residual_route_and_dirichlet_nodes():
    from diffnet_amd import helmholtz as hh
    from diffnet_amd import ops
    P, ngp, nelx, nely, B = 2, 3, 70, 9, 3
    m = hh_module(P, ngp, nelx, nely)
    shape = (B, 1, P * nely + 1, P * nelx + 1)
    u = smooth(shape, 90)
    m1 = torch.zeros(shape)
    m1[..., 0, :] = 1.0
    m2 = torch.zeros(shape)
    m2[..., :, 0] = 1.0
    m2[..., :, -1] = 1.0
    m1, m2 = m1.to(dev()), m2.to(dev())
    kw = dict(nu=cu(seeded(shape, 91, 0.5)), sigma=cu(seeded((1, 1, *shape[2:]), 92, 0.0)) * 30.0, bc=(m1, m2),
              bc_values=(cu(seeded(shape, 93, 0.5)), -0.75), f=cu(seeded(shape, 94, -0.5)) * 4.0)
    fixed = (m1 > 0.5) | (m2 > 0.5)
    R = hh.helmholtz_residual(m, u, **kw)
    Rc = hh.helmholtz_residual_composed(m, u, **kw)
    r64 = _float64(m, P, ngp, u, kw, ecoef=(0.0, 0.0, 0.0), ocoef=(1.0, 1.0, 1.0))
    dc, d64, c64 = _max_rel(R, Rc), _max_rel(R.double().cpu(), r64["out"]), _max_rel(Rc.double().cpu(), r64["out"])
    print("residual: fused-composed", dc, "fused-f64", d64, "composed-f64", c64)
    gtol = max(GTOL, 4 * c64)
    assert dc <= gtol and d64 <= gtol
    assert float(R[fixed].abs().max()) == 0.0 and float(R[~fixed].abs().max()) > 0
    # sumsq against sum R^2 of the composed R accumulated in fp64
    _, _, ss = ops.helmholtz_apply(m.geom, u, kw["nu"], kw["sigma"], kw["bc"], kw["bc_values"], kw["f"], None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0),
                                   want_out=False, want_energy=False, want_sumsq=True)
    ref = float((Rc.double() ** 2).sum())
    print("sumsq rel", abs(float(ss) - ref) / ref, "f64", abs(float(ss) - r64["sumsq"]) / r64["sumsq"])
    np.testing.assert_allclose(float(ss), ref, rtol=2e-5)
    # the loss and its gradient: two launches against autograd through the composed route
    for red in ("sum", "mean"):
        ua, ub = u.clone().requires_grad_(True), u.clone().requires_grad_(True)
        la = hh.helmholtz_residual_loss(m, ua, reduction=red, **kw)
        rc = hh.helmholtz_residual_composed(m, ub, **kw)
        lb = (rc ** 2).sum() if red == "sum" else (rc ** 2).mean()
        ga, = torch.autograd.grad(la, ua)
        gb, = torch.autograd.grad(lb, ub)
        l2, g2 = hh.helmholtz_residual_loss_and_grad(m, u, reduction=red, **kw)
        la, lb = la.detach(), lb.detach()
        print(red, "residual loss rel", abs(float(la) - float(lb)) / float(lb), "grad", _max_rel(ga, gb))
        np.testing.assert_allclose(float(la), float(lb), rtol=2e-5)
        np.testing.assert_allclose(float(l2), float(lb), rtol=2e-5)
        assert _max_rel(ga, gb) <= gtol and torch.equal(g2, ga)
        assert float(ga[fixed].abs().max()) == 0.0 and float(g2[fixed].abs().max()) == 0.0
    # the backward of R itself (a cotangent that is not R)
    ua, ub = u.clone().requires_grad_(True), u.clone().requires_grad_(True)
    cot = cu(seeded(shape, 95, -0.5))
    ga, = torch.autograd.grad((hh.helmholtz_residual(m, ua, **kw) * cot).sum(), ua)
    gb, = torch.autograd.grad((hh.helmholtz_residual_composed(m, ub, **kw) * cot).sum(), ub)
    assert _max_rel(ga, gb) <= gtol and float(ga[fixed].abs().max()) == 0.0
    # the energy's gradient is zero there too, and where both masks hold condition 2's value is the one used
    loss, g = hh.helmholtz_energy_loss_and_grad(m, u, **kw)
    assert float(g[fixed].abs().max()) == 0.0
    both = (m1 > 0.5) & (m2 > 0.5)
    l_a, g_a = hh.helmholtz_energy_loss_and_grad(m, u, **dict(kw, bc=(m1 * (~both).float(), m2)))
    assert torch.equal(l_a, loss) and torch.equal(g_a, g)
    l_b, _ = hh.helmholtz_energy_loss_and_grad(m, u, **dict(kw, bc=(m1, m2 * (~both).float())))
    assert not torch.equal(l_b, loss)


def test_helmholtz_bitwise_across_batch_sizes_plans_and_runs():
    from diffnet_amd import _lib, ops
    P, ngp, nelx, nely, B = 2, 3, 300, 37, 3          # Q = 301 thread columns: five one-wave chunks by default
    m = hh_module(P, ngp, nelx, nely)
    shape = (B, 1, P * nely + 1, P * nelx + 1)
    u = smooth(shape, 70)
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(9)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float()).to(torch.uint8)
    vals = (cu(seeded(shape, 80, -0.5)), 0.2)
    f = cu(seeded((B, ngp * ngp, nely, nelx), 81, -0.5))
    nu, sg = cu(seeded(shape, 82, 0.5)), cu(seeded(shape, 83, 0.0)) * 20.0
    kw = dict(energy_coef=(0.5, 0.5, 1.0), out_coef=(1.0, 1.0, 1.0), wscale=0.7, out_scale=0.01, want_sumsq=True)

    def run(uu=u, nn=nu, ss=sg, bc=(wall, blob), vv=vals, ff=f, **over):
        return ops.helmholtz_apply(m.geom, uu, nn, ss, bc, vv, None, ff, **dict(kw, **over))

    o, e, s = run()
    o2, e2, s2 = run()
    assert torch.equal(o, o2) and torch.equal(e, e2) and torch.equal(s, s2)       # run to run
    o3, e3, s3 = run(want_energy=False, want_sumsq=False)
    assert e3 is None and s3 is None and torch.equal(o3, o)
    o4, e4, s4 = run(want_out=False)
    assert o4 is None and torch.equal(e4, e) and torch.equal(s4, s)
    np.testing.assert_allclose(float(s), float(((o.double() / 0.01) ** 2).sum()), rtol=1e-6)
    # sample k of the batch launched alone: the same bits
    for k in range(B):
        one = lambda t: t[k:k + 1].contiguous()                                 # noqa: E731
        ok, _, _ = run(one(u), one(nu), one(sg), (one(wall), one(blob)), (one(vals[0]), 0.2), one(f), want_energy=False, want_sumsq=False)
        assert torch.equal(o[k:k + 1], ok), k
    # other launch plans (threads per workgroup, element rows per strip; two chunks of three and of four waves): the same bits
    try:
        for plan in ("64,1", "192,3", "256,64"):
            _lib.config_set("PLAN_FSDT", plan)
            op, ep, sp = run()
            assert torch.equal(op, o), plan
            np.testing.assert_allclose(float(ep), float(e), rtol=1e-12)
            np.testing.assert_allclose(float(sp), float(s), rtol=1e-12)
            op2, ep2, sp2 = run()
            assert torch.equal(ep2, ep) and torch.equal(sp2, sp), plan            # the sums: bitwise for a given mesh, batch and plan
    finally:
        _lib.config_set("PLAN_FSDT", "")
    o5, e5, s5 = run()
    assert torch.equal(o5, o) and torch.equal(e5, e) and torch.equal(s5, s)


def test_helmholtz_chained_with_strongform_and_poisson_on_one_stream():
    """A Helmholtz launch, a strong-form launch and a Poisson energy launch chained on one stream, repeatedly: every result equals its
    stand-alone value bitwise (the reduction workspaces are separate) and the workspace status is clean afterwards."""
    import ctypes as C
    from diffnet_amd import _lib, ops
    from diffnet_amd.helmholtz import helmholtz_residual_loss_and_grad
    m = hh_module(2, 3, 93, 24)
    shape = (2, 1, 49, 187)
    u = smooth(shape, 120)
    wall = boundary_mask(shape).to(dev())
    tm = module(dict(domain_size=65))
    tshape = (2, 1, 65, 65)
    tu, tnu, tf = (cu(seeded(tshape, 121 + i, 0.5 if i == 1 else -0.5)) for i in range(3))
    twall = boundary_mask(tshape).to(dev())

    def hh():
        return ops.helmholtz_apply(m.geom, u, None, 9.0, (wall, None), (1.0, 0.0), None, 0.3, want_sumsq=True)

    def hr():
        return helmholtz_residual_loss_and_grad(m, u, sigma=9.0, bc=(wall, None), bc_values=(1.0, 0.0), f_gp=0.3)

    def sf():
        return ops.strongform_apply(m.geom, u, (wall, None), (1.0, 0.0), None, 0.3, coef=(0.3, 1.0, 1.2, -0.05, 0.02, 1.0))

    def po():
        return tm.energy_loss_and_grad(tu, tnu, tf, dirichlet=[(twall, 0.0)])

    refs = dict(h=hh(), r=hr(), s=sf(), p=po())
    seq = []
    for _ in range(3):
        seq += [("h", hh()), ("s", sf()), ("p", po()), ("r", hr())]
    seq += [("h", hh()), ("h", hh()), ("p", po()), ("s", sf()), ("h", hh())]
    torch.cuda.synchronize()
    for k, r in seq:
        for a, b in zip(r, refs[k]):
            assert torch.equal(a, b), k
    ops.workspace_status()
    for (_, stream), ws in ops._HELMHOLTZ.ws.items():
        assert _lib.lib().dn_workspace_status(C.c_void_p(ws.data_ptr()), C.c_void_p(stream)) == 0


def test_helmholtz_graph_capture_replays_bitwise():
    from diffnet_amd.helmholtz import helmholtz_energy_loss_and_grad
    P, ngp, nelx, nely = 3, 4, 43, 15
    m = hh_module(P, ngp, nelx, nely)
    shape = (2, 1, P * nely + 1, P * nelx + 1)
    u = smooth(shape, 130)
    wall = boundary_mask(shape).to(dev())
    kw = dict(bc=(wall, wall[:1].to(torch.uint8)), bc_values=(cu(seeded((1, 1, *shape[2:]), 134, -0.5)), 0.0), f=cu(seeded(shape, 135, -0.5)),
              nu=cu(seeded(shape, 136, 0.5)), sigma=12.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):                     # warm-up on the capture stream: workspace, prepared call
            eager = helmholtz_energy_loss_and_grad(m, u, **kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):    # a single chain, no parallel branches
            static = helmholtz_energy_loss_and_grad(m, u, **kw)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static[0], eager[0]) and torch.equal(static[1], eager[1])


def test_helmholtz_gradient_routing_no_silent_zero_gradients():
    from diffnet_amd import helmholtz as hh
    from diffnet_amd._lib import DiffNetHipError
    m = module(dict(domain_size=17, fem_basis_deg=2))
    shape = (1, 1, 17, 17)
    u = smooth(shape, 1, (1.0, 1.0))
    wall = boundary_mask(shape).to(dev())
    mk = lambda seed, lo: cu(seeded(shape, seed, lo)).requires_grad_(True)      # noqa: E731
    for fn, comp in ((hh.helmholtz_energy_loss, hh.helmholtz_energy_loss_composed),
                     (hh.helmholtz_residual_loss, lambda *a, **k: (hh.helmholtz_residual_composed(*a, **k) ** 2).sum())):
        f, v1, nu, sg = mk(2, -0.5), mk(4, -0.5), mk(5, 0.5), mk(6, 0.0)
        fg = cu(seeded((9, 8, 8), 3, -0.5)).requires_grad_(True)
        for kw, wrt in ((dict(nu=nu, sigma=sg, bc=(wall, None), bc_values=(v1, 0.0), f=f), (nu, sg, v1, f)),
                        (dict(sigma=3.0, bc=(wall, None), bc_values=(0.5, 0.0), f_gp=fg), (fg,)),
                        (dict(sigma=sg), (sg,)), (dict(nu=nu, sigma=2.0, f_gp=1.0), (nu,))):
            ua, ub = u.clone().requires_grad_(True), u.clone().requires_grad_(True)
            ga = torch.autograd.grad(fn(m, ua, **kw), (ua, *wrt))
            gb = torch.autograd.grad(comp(m, ub, **kw), (ub, *wrt))
            for a, b in zip(ga, gb):
                assert a is not None and float(a.abs().max()) > 0 and _max_rel(a, b) <= GTOL
        # the fused route and the composed one are the same function of u
        ur = u.clone().requires_grad_(True)
        kd = dict(nu=nu.detach(), sigma=sg.detach(), bc=(wall, None), bc_values=(v1.detach(), 0.0), f=f.detach())
        l_f, l_c = fn(m, ur, **kd), comp(m, ur, **kd)
        g_f, = torch.autograd.grad(l_f, ur)
        g_c, = torch.autograd.grad(l_c, ur)
        assert _max_rel(g_f, g_c) <= GTOL
    # a backward with a scaled grad_output scales the saved gradient; a loss of a field without gradient computes none
    ur = u.clone().requires_grad_(True)
    ga, = torch.autograd.grad(3.0 * hh.helmholtz_energy_loss(m, ur, sigma=4.0, f_gp=1.0), ur)
    _, gb = hh.helmholtz_energy_loss_and_grad(m, u, sigma=4.0, f_gp=1.0)
    assert torch.equal(ga, 3.0 * gb)
    assert not hh.helmholtz_energy_loss(m, u, sigma=4.0).requires_grad
    with pytest.raises(DiffNetHipError):
        hh.helmholtz_energy_loss(m, u, bc=(boundary_mask(shape), None))           # a CPU mask
    with pytest.raises(ValueError):
        hh.helmholtz_energy_loss(m, u, bc=(None, None), bc_values=(cu(seeded(shape, 7)), 0.0))     # a value field without its mask
    with pytest.raises(ValueError):
        hh.helmholtz_energy_loss(m, u, f=cu(seeded(shape, 8)), f_gp=cu(seeded((9, 8, 8), 9)))       # two forcings


def test_helmholtz_example_fused_and_composed_agree():
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("ex_helmholtz_2d", os.path.join(here, "..", "examples", "helmholtz_2d.py"))
    ex = importlib.util.module_from_spec(spec)
    sys.modules["ex_helmholtz_2d"] = ex
    spec.loader.exec_module(ex)
    for case in ("mms", "ddelta"):
        mod = ex.Helmholtz(None, case, 17).to(dev())
        gross = _float64(mod, 1, 2, torch.ones((1, 1, 17, 17), device=dev()), dict(mod.inputs(), sigma=mod.khh ** 2))["gross"] / 16 ** 2
        for loss in ("energy", "residual"):
            _, hf = ex.run(case=case, n=17, steps=4, loss=loss, mode="fused", verbose=False)
            _, hc = ex.run(case=case, n=17, steps=4, loss=loss, mode="composed", verbose=False)
            print(case, loss, hf, hc, "gross", gross)
            assert hf[-1] < hf[0] and hc[-1] < hc[0], (case, loss)
            # the first evaluation: the energy within ETOL of the gross sum, sum R^2 within 2e-5 relative
            assert abs(hf[0] - hc[0]) <= ETOL * (gross if loss == "energy" else abs(hc[0])), (case, loss)


def test_helmholtz_scripts_own_size():
    """One evaluation at 64^2 Q1 on the RectangleHelmholtzManufactured sample against the float64 restatement."""
    from diffnet_amd.datasets.single_instances.rectangles import RectangleHelmholtzManufactured
    from diffnet_amd.helmholtz import helmholtz_coefficients, helmholtz_energy_loss_and_grad
    n = 64
    ds = RectangleHelmholtzManufactured(domain_size=n)
    inp, frc = ds[0]
    inp, frc = torch.as_tensor(np.asarray(inp), dtype=torch.float32)[None].to(dev()), torch.as_tensor(np.asarray(frc), dtype=torch.float32)[None].to(dev())
    m = module(dict(domain_size=n))
    u = smooth((1, 1, n, n), 140, (1.0, 1.0))
    kw = dict(nu=inp[:, 0:1].contiguous(), bc=(inp[:, 1:2].contiguous(), inp[:, 2:3].contiguous()), bc_values=(1.0, 0.0),
              f=frc.reshape(1, 1, n, n).contiguous())
    coef = helmholtz_coefficients(ds.khh)
    loss, g = helmholtz_energy_loss_and_grad(m, u, **kw, **coef)
    nel = (n - 1) ** 2
    r64 = _float64(m, 1, 2, u, dict(kw, sigma=coef["sigma"]), out_scale=1.0 / nel)
    print("64^2: loss / gross", abs(float(loss) - r64["energy"] / nel) / (r64["gross"] / nel), "grad", _max_rel(g.double().cpu(), r64["out"]))
    assert abs(float(loss) - r64["energy"] / nel) <= ETOL * r64["gross"] / nel
    assert _max_rel(g.double().cpu(), r64["out"]) <= GTOL
