"""GPU tests of the fused 3-D eikonal weak-form residual and its VJP (dn_eikonal3d_apply, csrc/eikonal3d.hip; diffnet_amd/eikonal.py on a
DiffNet3DFEM): against the reference fixtures (tests/golden/loss_eikonal3d_*.npz, the reference script's own loss body), against the same
functions composed from the drop-in operators on every compile-time form and rule, on ragged meshes around the seams of the launch plan,
against the float64 restatement of tests/test_eikonal3d_host.py; the VJP launch with a random cotangent, the Dirichlet nodes, bitwise
independence of batch and launch plan, isolation of its reduction workspace from 2-D eikonal and 3-D Poisson launches, graph capture,
gradient routing and the example."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from test_eikonal3d_host import FIXTURES, default_plan, eikonal3d_t64, ek3_mesh, fixture_case, fixture_norm64
from test_gpu_helmholtz import _fixed, _max_rel
from test_gpu_parity import boundary_mask, close, cu, dev, load, module, seeded
from test_transport_host import GRAD_AREL, GRAD_RTOL, LOSS_RTOL

pytestmark = pytest.mark.gpu

# SHAPES: (ngp, nelx, nely, nelz, B).  The default plan (include/diffnet_hip.h, dn_eikonal3d_apply) has tiles 16 threads wide that
# overlap by one thread column (a seam from 17 node columns on: nelx 16, 17, 31, 33; none at 15), tiles 4 .. 16 rows high that overlap
# by one row (a seam at nely 16 and 17: two tiles of 12 rows) and strips of at least 4 element planes that recompute one layer (a
# seam at nelz 5, 9, 13; none at 1, 3, 4).  Every rule meets every seam kind at least once, and the one-element mesh.
# The tolerances of the 2-D file (tests/test_gpu_eikonal.py): R within 1e-4 of its largest entry, the loss within 2e-5 relative, the
# gradient within 1e-4 of its largest entry.
# Largest distances measured over all meshes and cases (the test prints each): R 5.5e-7, loss 2.4e-7 (norm) / 4.5e-7 (sumsq), gradient
# 6.6e-7, VJP with a random cotangent 3.3e-7; against the float64 restatement: R 2.8e-7, norm 1.3e-7, gradient 2.3e-7.
RTOL_R, RTOL_LOSS, RTOL_G = 1e-4, 2e-5, 1e-4
SHAPES = [(2, 1, 1, 1, 1), (2, 2, 3, 1, 2), (2, 15, 4, 5, 1), (2, 16, 15, 4, 2), (2, 17, 16, 3, 1), (2, 33, 5, 9, 3), (2, 31, 17, 13, 1),
          (3, 2, 3, 1, 2), (3, 17, 16, 3, 1), (3, 33, 5, 9, 3),
          (4, 15, 4, 5, 1), (4, 17, 16, 3, 1), (4, 31, 17, 13, 1)]
LENGTHS = (1.0, 0.8, 1.3)


def ek3_module(ngp, nelx, nely, nelz, lengths=LENGTHS, deg=1):
    sizes = (deg * nelx + 1, deg * nely + 1, deg * nelz + 1)
    return module(dict(nsd=3, domain_sizes=sizes, domain_lengths=lengths, domain_size=sizes[0], domain_length=lengths[0], fem_basis_deg=deg,
                       ngp_1d=ngp))


def field(shape, seed, lengths=LENGTHS):
    """The fixtures' scaling: the distance to a sphere (|grad u| = 1) + h x seeded noise in (-1/2, 1/2), h the node spacing along x"""
    B, _, nz, ny, nx = shape
    x, y, z = (torch.linspace(0, L, n) for L, n in zip(lengths, (nx, ny, nz)))
    r = torch.sqrt((x[None, None, :] - 0.5 * lengths[0]) ** 2 + (y[None, :, None] - 0.5 * lengths[1]) ** 2 + (z[:, None, None] - 0.5 * lengths[2]) ** 2) - 0.3
    h = lengths[0] / max(nx - 1, 1)
    return cu(r + h * (seeded(shape, seed) - 0.5))


def test_shapes_sit_on_the_seams_of_the_default_plan():
    """(no GPU work) the comment above, checked against the plan the host test restates"""
    seams = {}
    for ngp, nelx, nely, nelz, B in SHAPES:
        TX, TY, R = default_plan(ek3_mesh((nelx + 1, nely + 1, nelz + 1), ngp, B))
        s = seams.setdefault(ngp, set())
        s |= {"column"} if nelx + 1 > TX else set()
        s |= {"row"} if nely + 1 > TY else set()
        s |= {"layer"} if nelz > R else set()
    assert all(seams[ngp] == {"column", "row", "layer"} for ngp in (2, 3, 4)), seams


@pytest.mark.parametrize("name", FIXTURES)
def test_eikonal3d_vs_reference_golden(name):
    from diffnet_amd.eikonal import eikonal_coefficients, eikonal_loss, eikonal_loss_and_grad, eikonal_residual
    z = load(name)
    c = fixture_case(z)
    m = module(eval(str(z["kwargs"])))
    coef = eikonal_coefficients(c["tau"])
    assert coef["sq"] == c["sq"] and abs((0.5 * m.hx) * (0.5 * m.hy) * (0.5 * m.hz) - c["wscale"]) <= 1e-12
    u = cu(z["u"]).requires_grad_(True)
    loss = eikonal_loss(m, u, kind="norm", **coef)
    g, = torch.autograd.grad(loss, u)
    ref, pt, nrm = z["grad"], float(z["point_terms"]), fixture_norm64(z)
    print(name, "||R|| rel", abs(float(loss.detach()) - nrm) / nrm, "grad", float(np.abs(g.cpu().numpy() - ref).max() / np.abs(ref).max()))
    np.testing.assert_allclose(float(loss.detach()), nrm, rtol=LOSS_RTOL)
    np.testing.assert_allclose(float(loss.detach()) + pt, float(z["loss"]), rtol=LOSS_RTOL)
    close(g, ref, rtol=GRAD_RTOL, arel=GRAD_AREL)
    l2, g2 = eikonal_loss_and_grad(m, u.detach(), kind="norm", **coef)
    assert l2.dtype == torch.float32 and l2.dim() == 0
    np.testing.assert_allclose(float(l2), nrm, rtol=LOSS_RTOL)
    close(g2, ref, rtol=GRAD_RTOL, arel=GRAD_AREL)
    assert torch.equal(g2, g) and torch.equal(l2, loss.detach())
    close(eikonal_residual(m, u.detach(), **coef)[0, 0], z["R1"], rtol=GRAD_RTOL, arel=GRAD_AREL)


def _cases(shape, ngp):
    """(name, kwargs): every compile-time form (mask none / constants / value fields; forcing constant / nodal / Gauss points, shared and
    per sample) at least once; masks fp32 / uint8 / bool, shared and per sample, overlapping; tau = 0 and tau = 0.25"""
    B, _, nz, ny, nx = shape
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(3)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float())
    shared = wall[:1].contiguous()
    G, eshape = ngp ** 3, (nz - 1, ny - 1, nx - 1)
    f_sh = cu(seeded((G, *eshape), 20, 0.5))
    f_b = cu(seeded((B, G, *eshape), 21, 0.5))
    fn_sh = cu(seeded((1, 1, nz, ny, nx), 22, 0.5))
    fn_b = cu(seeded(shape, 23, 0.5))
    vfield = 0.3 * cu(seeded(shape, 30, -0.5))
    vshared = 0.3 * cu(seeded((1, 1, nz, ny, nx), 31, -0.5))
    return [
        ("no masks, the scripts' constants", dict(tau=0.25)),
        ("no masks, nodal forcing shared, unstabilised", dict(f=fn_sh, tau=0.0, sq=1.0)),
        ("no masks, gp forcing shared", dict(f_gp=f_sh, tau=0.25)),
        ("fp32 shared + per sample, constants, gp forcing per sample", dict(bc=(shared, blob), bc_values=(0.1, 0.0), f_gp=f_b, tau=0.25)),
        ("fp32 overlapping, value fields, gp forcing shared", dict(bc=(wall, blob), bc_values=(vfield, vshared), f_gp=f_sh, tau=0.25, sq=0.9)),
        ("u8 per sample + bool shared, value field + constant, nodal forcing per sample", dict(bc=(blob.to(torch.uint8), shared.bool()), bc_values=(vshared, 0.05), f=fn_b, tau=0.25)),
        ("bool only condition 2, constant forcing, tau 0", dict(bc=(None, blob.bool()), bc_values=(0.0, -0.1), f_gp=0.7, tau=0.0)),
        ("u8 shared, nodal forcing shared", dict(bc=(shared.to(torch.uint8), None), bc_values=(0.1, 0.0), f=fn_sh, tau=0.25)),
        ("u8 shared, value field per sample, the scripts' constants", dict(bc=(shared.to(torch.uint8), None), bc_values=(vfield, 0.0), tau=0.25)),
    ]


@pytest.mark.parametrize("ngp,nelx,nely,nelz,B", SHAPES)
def test_eikonal3d_fused_matches_composed(ngp, nelx, nely, nelz, B):
    from diffnet_amd import eikonal as ek
    m = ek3_module(ngp, nelx, nely, nelz)
    shape = (B, 1, nelz + 1, nely + 1, nelx + 1)
    u = field(shape, 10)
    cot = cu(seeded(shape, 11, -0.5))
    for name, kw in _cases(shape, ngp):
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
            la, lb = float(la.detach()), float(lb.detach())      # both are 0 where every node is a Dirichlet node (the one-element mesh with the wall)
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
        print((ngp, nelx, nely, nelz, B), name, "R", dist[0], "| norm: loss", dist[1], "grad", dist[2], "| sumsq: loss", dist[3], "grad", dist[4], "| vjp", dv)
        assert dv <= RTOL_G, (name, "vjp", dv)
        assert float(ga[fixed].abs().max() if fixed.any() else 0.0) == 0.0, name


@pytest.mark.parametrize("ngp,nelx,nely,nelz,B", [(2, 3, 2, 4, 1), (3, 5, 3, 2, 2), (4, 3, 2, 4, 1)])
def test_eikonal3d_fused_matches_float64_restatement(ngp, nelx, nely, nelz, B):
    """Against a mistake both GPU routes could share (wscale, the Gauss-point order of f_gp, the condition order)"""
    from diffnet_amd import eikonal as ek
    m = ek3_module(ngp, nelx, nely, nelz)
    shape = (B, 1, nelz + 1, nely + 1, nelx + 1)
    u = field(shape, 40)
    rs = torch.Generator().manual_seed(41)
    m1, m2 = torch.rand(shape, generator=rs) < 0.2, torch.rand(shape, generator=rs) < 0.2
    m1[:, :, 0, 0, 0] = m2[:, :, 0, 0, 0] = True
    v1, v2 = 0.3 * seeded(shape, 42, -0.5), 0.3 * seeded(shape, 43, -0.5)
    fn = seeded(shape, 44, 0.5)
    fg = seeded((B, ngp ** 3, nelz, nely, nelx), 45, 0.5)
    hx, hy, hz = m.hx, m.hy, m.hz
    for what, fkw, f64 in (("nodal forcing", dict(f=cu(fn)), fn), ("gp forcing", dict(f_gp=cu(fg)), fg)):
        kw = dict(bc=(m1.to(dev()), cu(m2.float())), bc_values=(cu(v1), cu(v2)), tau=0.25, sq=1.4, wscale=0.8, **fkw)
        R = ek.eikonal_residual(m, u, **kw)
        loss, g = ek.eikonal_loss_and_grad(m, u, **kw)
        fb = lambda b: (f64[b, 0] if f64.dim() == 5 and f64.shape[1] == 1 else f64[b]).double()      # noqa: E731
        us = [u[b, 0].double().cpu().requires_grad_(True) for b in range(B)]
        Rs = [eikonal3d_t64(us[b], hx, hy, hz, ngp, 0.25, 1.4, fb(b), 0.8, (m1[b, 0], m2[b, 0]), (v1[b, 0].double(), v2[b, 0].double())) for b in range(B)]
        for b in range(B):
            Rb = Rs[b].detach()
            d = float((R[b, 0].double().cpu() - Rb).abs().max() / Rb.abs().max())
            print((ngp, nelx, nely, nelz, B), what, "sample", b, "R", d)
            assert d <= RTOL_R, (what, b, d)
            assert float(R[b, 0][(m1 | m2)[b, 0].to(dev())].abs().max()) == 0.0
        # the batch norm and its gradient
        nrm = torch.sqrt(sum((r ** 2).sum() for r in Rs))
        gs = torch.stack(torch.autograd.grad(nrm, us))[:, None]
        nrm = float(nrm.detach())
        dl, dg = abs(float(loss) - nrm) / nrm, _max_rel(g.double().cpu(), gs)
        print((ngp, nelx, nely, nelz, B), what, "norm", dl, "gradient", dg)
        assert dl <= RTOL_LOSS and dg <= RTOL_G, (what, dl, dg)


def test_eikonal3d_dirichlet_nodes_and_condition_order():
    from diffnet_amd import eikonal as ek
    ngp, nelx, nely, nelz, B = 3, 20, 9, 6, 3
    m = ek3_module(ngp, nelx, nely, nelz)
    shape = (B, 1, nelz + 1, nely + 1, nelx + 1)
    u = field(shape, 90)
    m1 = torch.zeros(shape)
    m1[..., 0, :, :] = 1.0
    m1[..., :, 0, :] = 1.0
    m2 = torch.zeros(shape)
    m2[..., :, :, 0] = 1.0
    m2[..., :, :, -1] = 1.0
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


def test_eikonal3d_bitwise_across_batch_sizes_plans_and_runs():
    from diffnet_amd import _lib, ops
    ngp, nelx, nely, nelz, B = 2, 40, 21, 11, 3        # 41 x 22 x 12 nodes: 3 chunks x 2 tiles x 3 strips by default
    m = ek3_module(ngp, nelx, nely, nelz)
    shape = (B, 1, nelz + 1, nely + 1, nelx + 1)
    u = field(shape, 70)
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(9)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float()).to(torch.uint8)
    vals = (0.3 * cu(seeded(shape, 80, -0.5)), 0.1)
    f = cu(seeded((B, ngp ** 3, nelz, nely, nelx), 81, 0.5))
    cot = cu(seeded(shape, 82, -0.5))
    kw = dict(tau=0.25, wscale=0.7)

    def fwd(uu=u, bc=(wall, blob), vv=vals, ff=f, **over):
        return ops.eikonal3d_apply(m.geom, uu, bc, vv, None, ff, **{**kw, **dict(want_sumsq=True, want_norm=True), **over})

    def vjp(uu=u, bc=(wall, blob), vv=vals, cc=cot):
        return ops.eikonal3d_apply(m.geom, uu, bc, vv, cot=cc, **kw)[0]

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
    # other launch plans (tile width and height, element planes per strip): every seam moves, the same bits
    try:
        for plan in ("8,8,1,4", "16,8,1,2", "16,16,1,64", "32,4,1,3", "4,16,1,5"):
            _lib.config_set("PLAN3D", plan)
            op, sp, _ = fwd()
            assert torch.equal(op, o) and torch.equal(vjp(), g), plan
            np.testing.assert_allclose(float(sp), float(s), rtol=1e-12)
            assert torch.equal(fwd()[1], sp), plan                                # the sum: bitwise for a given mesh, batch and plan
    finally:
        _lib.config_set("PLAN3D", "")
    o5, s5, n5 = fwd()
    assert torch.equal(o5, o) and torch.equal(s5, s) and torch.equal(n5, nr)


def test_eikonal3d_workspace_is_isolated_from_other_operators():
    """3-D eikonal launches interleaved on one stream with 2-D eikonal launches and a 3-D Poisson residual loss, repeatedly: every result
    equals its stand-alone value bitwise (the reduction workspaces are separate) and the workspace status is clean afterwards."""
    import ctypes as C
    from diffnet_amd import _lib, ops
    from diffnet_amd.eikonal import eikonal_loss_and_grad
    m = ek3_module(2, 20, 17, 9)
    shape = (2, 1, 10, 18, 21)
    u = field(shape, 120)
    wall = boundary_mask(shape).to(dev())
    m2 = module(dict(domain_size=33))
    u2 = cu(seeded((2, 1, 33, 33), 121, -0.5))

    def ek():
        return eikonal_loss_and_grad(m, u, bc=(wall, None), bc_values=(0.1, 0.0), tau=0.25)

    def es():
        return ops.eikonal3d_apply(m.geom, u, (wall, None), (0.1, 0.0), tau=0.25, want_sumsq=True, want_norm=True)

    def e2():
        return eikonal_loss_and_grad(m2, u2, tau=0.25)

    def po():
        return (m.residual_loss(u, dirichlet=[(wall, 0.1)]).detach().reshape(1),)

    refs = dict(e=ek(), s=es(), t=e2(), p=po())
    seq = []
    for _ in range(3):
        seq += [("e", ek()), ("t", e2()), ("s", es()), ("p", po())]
    seq += [("e", ek()), ("e", ek()), ("p", po()), ("s", es())]
    torch.cuda.synchronize()
    for k, r in seq:
        for a, b in zip(r, refs[k]):
            assert torch.equal(a, b), k
    ops.workspace_status()
    assert ops._EIKONAL3D.ws and all(w is not v for w in ops._EIKONAL3D.ws.values() for v in ops._EIKONAL.ws.values())
    for (_, stream), ws in ops._EIKONAL3D.ws.items():
        assert _lib.lib().dn_workspace_status(C.c_void_p(ws.data_ptr()), C.c_void_p(stream)) == 0


def test_eikonal3d_graph_capture_replays_bitwise():
    from diffnet_amd.eikonal import eikonal_loss_and_grad
    ngp, nelx, nely, nelz = 3, 19, 17, 9
    m = ek3_module(ngp, nelx, nely, nelz)
    shape = (2, 1, nelz + 1, nely + 1, nelx + 1)
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


def test_eikonal3d_gradient_routing_no_silent_zero_gradients():
    from diffnet_amd import eikonal as ek
    from diffnet_amd._lib import DiffNetHipError
    m = module(dict(domain_size=9, nsd=3))
    shape = (1, 1, 9, 9, 9)
    u = field(shape, 1, (1.0, 1.0, 1.0))
    wall = boundary_mask(shape).to(dev())
    mk = lambda seed, lo: cu(seeded(shape, seed, lo)).requires_grad_(True)      # noqa: E731
    f, v1 = mk(2, 0.5), mk(4, -0.5)
    fg = cu(seeded((8, 8, 8, 8), 3, 0.5)).requires_grad_(True)
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
        ek.eikonal_loss(m, u, f=cu(seeded(shape, 8)), f_gp=cu(seeded((8, 8, 8, 8), 9)))       # two forcings
    # a 3-D Q2 mesh: the fused route raises and names the composed one, which works
    mq = module(dict(domain_size=9, nsd=3, fem_basis_deg=2))
    for fn in (ek.eikonal_residual, ek.eikonal_loss, ek.eikonal_loss_and_grad):
        with pytest.raises(DiffNetHipError, match="eikonal_residual_composed"):
            fn(mq, u, tau=0.25)
    ur = u.clone().requires_grad_(True)
    Rq = ek.eikonal_residual_composed(mq, ur, bc=(wall, None), bc_values=(0.1, 0.0), tau=0.25)
    gq, = torch.autograd.grad(torch.norm(Rq), ur)
    assert Rq.shape == u.shape and bool(torch.isfinite(Rq).all()) and float(Rq.abs().max()) > 0 and float(gq.abs().max()) > 0
    assert float(Rq[wall > 0.5].abs().max()) == 0.0


def test_eikonal3d_example_fused_and_composed_agree():
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("ex_eikonal_3d", os.path.join(here, "..", "examples", "eikonal_3d.py"))
    ex = importlib.util.module_from_spec(spec)
    sys.modules["ex_eikonal_3d"] = ex
    spec.loader.exec_module(ex)
    _, hf = ex.run(n=17, steps=4, optimizer="lbfgs", mode="fused", verbose=False)
    _, hc = ex.run(n=17, steps=4, optimizer="lbfgs", mode="composed", verbose=False)
    print("lbfgs", "fused", hf, "composed", hc)
    assert hf[-1] < hf[0] and hc[-1] < hc[0]
    assert abs(hf[0] - hc[0]) <= 1e-4 * abs(hc[0]) and abs(hf[-1] - hc[-1]) <= 1e-4 * abs(hc[-1])
