"""GPU tests of the fused 2-D Navier-Stokes (VMS) residual (dn_ns_apply, csrc/navier_stokes.hip; diffnet_amd/navier_stokes.py): against the
reference fixtures (tests/golden/loss_ns_*.npz, the reference scripts' own residual bodies), against the same residuals composed from the
drop-in operators on every mask / value / forcing form and on the meshes where marching kernels go wrong, the VJP launch against autograd
through the composition and against the float64 restatement, batch independence, the in-kernel norms and the zero cases, isolation of its
reduction workspace from a deferred FSDT pair and from Stokes launches, graph capture, and the lid-driven-cavity example."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import boundary_mask, close, cu, dev, load, module, seeded
from test_ns_host import ns_torch

pytestmark = pytest.mark.gpu

FIXTURES = ["ldc_n17", "ldc_n33_g3", "fps_rect"]
MESHES = [(65, 65, 2, 2), (257, 257, 3, 3), (130, 47, 2, 4), (33, 129, 1, 3), (64, 5, 3, 2), (2, 2, 2, 4)]


def fixture_inputs(z):
    m = module(eval(str(z["kwargs"])))
    inp = cu(z["inputs"])
    bc = tuple(inp[:, 2 + k:3 + k].contiguous() for k in range(3))
    vals = tuple(cu(z[n]).reshape(1, 1, *z[n].shape) for n in ("u_bc", "v_bc", "p_bc"))
    f_gp = (cu(z["f1"]), cu(z["f2"])) if np.abs(z["f1"]).max() > 0 or np.abs(z["f2"]).max() > 0 else None
    kw = dict(bc_values=vals, visco=float(z["visco"]), f_gp=f_gp, wscale=float(z["wscale"]), tau_h=tuple(float(x) for x in z["tau_h"]))
    return m, bc, kw


@pytest.mark.parametrize("tag", FIXTURES)
def test_ns_vs_reference_golden(tag):
    from diffnet_amd.navier_stokes import ns_loss, ns_residuals
    z = load(f"loss_ns_{tag}.npz")
    m, bc, kw = fixture_inputs(z)
    fields = [cu(z[n]).requires_grad_(True) for n in ("u", "v", "p")]
    Rs = ns_residuals(m, *fields, bc, **kw)
    for i, R in enumerate(Rs):
        close(R, z[f"R{i + 1}"], rtol=1e-4, arel=1e-5, msg=f"R{i + 1}")
    norms = ns_loss(m, *fields, bc, **kw)
    for i, nv in enumerate(norms):
        np.testing.assert_allclose(float(nv), float(z["norms"][i]), rtol=1e-4)
        gs = torch.autograd.grad(nv, fields, retain_graph=True)
        ref = z[f"grad_norm{i + 1}"]
        for q, (gq, rq) in enumerate(zip(gs, ref)):
            close(gq, rq, rtol=1e-4, arel=1e-5 * float(np.abs(ref).max()) / max(float(np.abs(rq).max()), 1e-30), msg=f"grad {i} {q}")


def rect_module(nx, ny, ngp, lengths=(1.0, 0.7)):
    return module(dict(domain_sizes=(nx, ny), domain_lengths=lengths, domain_size=nx, domain_length=lengths[0], ngp_1d=ngp))


def _max_rel(a, b):
    scale = max(float(b.abs().max()), float(a.abs().max()), 1e-30)
    return float((a - b).abs().max()) / scale


def _cases(shape, ngp):
    B, _, ny, nx = shape
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(3)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float())
    shared = wall[:1].contiguous()
    G, eshape = ngp * ngp, (ny - 1, nx - 1)
    f_sh = cu(seeded((G, *eshape), 20, -0.5))
    f_b = cu(seeded((B, G, *eshape), 21, -0.5))
    vfield = cu(seeded(shape, 30, -0.5))
    vshared = cu(seeded((1, 1, ny, nx), 31, -0.5))
    return [
        ("fp32 shared, constants, no forcing", shared, (0.3, -0.2, 0.1), None),
        ("fp32 per sample, value fields, gp forcing shared", (wall, blob, shared), (vfield, vshared, 0.5), (f_sh, f_sh)),
        ("u8 per sample, None entry, batched forcing", (blob.to(torch.uint8), None, shared.to(torch.uint8)), (vshared, 0.0, vfield), (f_b, None)),
        ("bool, constant forcing", (wall.bool(), wall.bool(), blob.bool()), (0.0, 1.0, vshared), (0.7, -1.3)),
        ("no masks, mixed forcing", None, (0.0, 0.0, 0.0), (-0.4, f_b)),
    ]


# Tolerance 1e-4 of the largest residual (Stokes: 2e-5): the weak forms are products of up to four fp32 Gauss-point quantities (tau_m^2 r r
# Nx) whose two implementations round in different orders, and the nodes that take the largest values are the ones where the terms cancel least.
@pytest.mark.parametrize("nx,ny,B,ngp", MESHES)
def test_ns_fused_matches_composed(nx, ny, B, ngp):
    from diffnet_amd.navier_stokes import ns_residuals, ns_residuals_composed
    m = rect_module(nx, ny, ngp)
    shape = (B, 1, ny, nx)
    fields = [cu(seeded(shape, 10 + i, -0.5)) * 2.0 for i in range(3)]
    for name, bc, vals, f in _cases(shape, ngp):
        kw = dict(bc_values=vals, visco=0.05, f_gp=f)
        got = ns_residuals(m, *fields, bc, **kw)
        ref = ns_residuals_composed(m, *fields, bc, **kw)
        for k in range(3):
            assert _max_rel(got[k], ref[k]) <= 1e-4, (name, k, _max_rel(got[k], ref[k]))


@pytest.mark.parametrize("nx,ny,B,ngp", MESHES)
def test_ns_vjp_launch_matches_autograd_of_composed(nx, ny, B, ngp):
    from diffnet_amd.navier_stokes import ns_loss, ns_residuals, ns_residuals_composed
    m = rect_module(nx, ny, ngp)
    shape = (B, 1, ny, nx)
    x = [cu(seeded(shape, 40 + i, -0.5)) * 2.0 for i in range(3)]
    for name, bc, vals, f in _cases(shape, ngp)[1:4]:
        kw = dict(bc_values=vals, visco=0.05, f_gp=f)
        # residual cotangents
        cot = [cu(seeded(shape, 50 + i, -0.5)) for i in range(3)]
        fa = [t.clone().requires_grad_(True) for t in x]
        fb = [t.clone().requires_grad_(True) for t in x]
        ga = torch.autograd.grad(ns_residuals(m, *fa, bc, **kw), fa, cot)
        gb = torch.autograd.grad(ns_residuals_composed(m, *fb, bc, **kw), fb, cot, allow_unused=True)
        for q in range(3):
            ref = torch.zeros_like(ga[q]) if gb[q] is None else gb[q]
            assert _max_rel(ga[q], ref) <= 1e-4, (name, "cot", q, _max_rel(ga[q], ref))
        # the three norms, each through the scaled VJP launch
        na = ns_loss(m, *fa, bc, **kw)
        nb = [torch.norm(R) for R in ns_residuals_composed(m, *fb, bc, **kw)]
        for k in range(3):
            np.testing.assert_allclose(float(na[k]), float(nb[k]), rtol=2e-5)
            ga = torch.autograd.grad(na[k], fa, retain_graph=True)
            gb = torch.autograd.grad(nb[k], fb, retain_graph=True, allow_unused=True)
            for q in range(3):
                ref = torch.zeros_like(ga[q]) if gb[q] is None else gb[q]
                assert _max_rel(ga[q], ref) <= 1e-4, (name, k, q, _max_rel(ga[q], ref))


@pytest.mark.parametrize("ngp", [2, 3, 4])
def test_ns_vjp_launch_matches_float64_restatement(ngp):
    from diffnet_amd.navier_stokes import ns_residuals
    ny, nx = 9, 12
    m = rect_module(nx, ny, ngp)
    rs = np.random.default_rng(7 + ngp)
    fields = [2 * rs.random((ny, nx)) - 1 for _ in range(3)]
    cot = [2 * rs.random((ny, nx)) - 1 for _ in range(3)]
    masks = [rs.random((ny, nx)) < 0.3, boundary_mask((1, 1, ny, nx))[0, 0].numpy() > 0.5, None]
    G = ngp * ngp
    f1, f2 = rs.random((G, ny - 1, nx - 1)) - 0.5, rs.random((G, ny - 1, nx - 1)) - 0.5
    vals = [0.3, 2 * rs.random((ny, nx)) - 1, 0.0]
    c = dict(masks=masks, vals=vals, f1=f1, f2=f2, visco=0.05, J=(0.5 * m.hx) * (0.5 * m.hy), hx=m.hx, hy=m.hy, tau_h=(m.hx, m.hy), cinv=36.0,
             ngp=ngp)
    ft = [torch.tensor(f, requires_grad=True) for f in fields]
    Rr = ns_torch(*ft, **c)
    gr = torch.autograd.grad(Rr, ft, [torch.tensor(x) for x in cot])
    bc = tuple(None if mk is None else cu(mk.astype(np.float32)).reshape(1, 1, ny, nx) for mk in masks)
    kw = dict(bc_values=(0.3, cu(vals[1].astype(np.float32)).reshape(1, 1, ny, nx), 0.0), visco=0.05,
              f_gp=(cu(f1.astype(np.float32)), cu(f2.astype(np.float32))))
    fg = [cu(f.astype(np.float32)).reshape(1, 1, ny, nx).requires_grad_(True) for f in fields]
    Rg = ns_residuals(m, *fg, bc, **kw)
    for k in range(3):
        assert _max_rel(Rg[k][0, 0].double().cpu(), Rr[k].detach()) <= 1e-4, k
    gg = torch.autograd.grad(Rg, fg, [cu(x.astype(np.float32)).reshape(1, 1, ny, nx) for x in cot])
    for q in range(3):
        assert _max_rel(gg[q][0, 0].double().cpu(), gr[q]) <= 1e-4, q


def test_ns_batch_samples_are_independent_bitwise():
    from diffnet_amd import ops
    m = rect_module(257, 129, 3)
    B = 3
    shape = (B, 1, 129, 257)
    fields = [cu(seeded(shape, 70 + i, -0.5)) for i in range(3)]
    cot = [cu(seeded(shape, 75 + i, -0.5)) for i in range(3)]
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(9)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float())
    vals = (cu(seeded(shape, 80, -0.5)), 0.2, 0.0)
    f = (cu(seeded((B, 9, 128, 256), 81, -0.5)), 0.3)
    bc = (wall, blob, blob.to(torch.uint8))
    kw = dict(visco=0.05, wscale=0.2)
    outs, _, norms = ops.ns_apply(m.geom, *fields, bc, vals, f_gp=f, want_norms=True, **kw)
    grads, _ = ops.ns_apply(m.geom, *fields, bc, vals, f_gp=f, cot=cot, want_sums=False, **kw)
    for b in range(B):
        sl = slice(b, b + 1)
        one = lambda ts: [t[sl].contiguous() for t in ts]                      # noqa: E731
        bcb = (wall[sl].contiguous(), blob[sl].contiguous(), blob[sl].to(torch.uint8))
        valb = (vals[0][sl].contiguous(), 0.2, 0.0)
        fb = (f[0][sl].contiguous(), 0.3)
        ob, _ = ops.ns_apply(m.geom, *one(fields), bcb, valb, f_gp=fb, want_sums=False, **kw)
        gb, _ = ops.ns_apply(m.geom, *one(fields), bcb, valb, f_gp=fb, cot=one(cot), want_sums=False, **kw)
        for k in range(3):
            assert torch.equal(outs[k][sl], ob[k]), (b, k)
            assert torch.equal(grads[k][sl], gb[k]), (b, k)


def test_ns_norms_zero_residual_and_loss_and_grad():
    from diffnet_amd import ops
    from diffnet_amd.navier_stokes import ns_loss, ns_loss_and_grad, ns_total_loss
    m = rect_module(97, 65, 2)
    B = 2
    shape = (B, 1, 65, 97)
    fields = [cu(seeded(shape, 90 + i, -0.5)) for i in range(3)]
    wall = boundary_mask(shape).to(dev())
    kw = dict(bc_values=(0.1, 0.0, 0.0), visco=0.05, f_gp=(0.3, -0.2))
    outs, sums, norms = ops.ns_apply(m.geom, *fields, wall[:1].contiguous(), kw["bc_values"], kw["visco"], kw["f_gp"],
                                     (0.5 * m.hx) * (0.5 * m.hy), want_norms=True)
    ref = np.array([float((o.double() ** 2).sum()) for o in outs])
    np.testing.assert_allclose(sums.cpu().numpy(), ref, rtol=1e-6)          # (per-lane partial sums are fp32, the rest fp64)
    np.testing.assert_allclose(norms.cpu().numpy(), np.sqrt(ref), rtol=1e-6)
    # every node Dirichlet with zero values: zero residuals, zero norms, zero (not NaN) gradients
    ones = torch.ones((1, 1, 65, 97), device=dev())
    fz = [t.clone().requires_grad_(True) for t in fields]
    nz = ns_loss(m, *fz, ones)
    assert all(float(x) == 0.0 for x in nz)
    g = torch.autograd.grad(sum(nz), fz)
    assert all(torch.isfinite(t).all() and float(t.abs().max()) == 0.0 for t in g)
    # ns_loss_and_grad == autograd of ns_total_loss (and weights)
    fa = [t.clone().requires_grad_(True) for t in fields]
    total = ns_total_loss(m, *fa, (wall, wall, None), **kw)
    total.backward()
    n2, g2 = ns_loss_and_grad(m, *fields, (wall, wall, None), **kw)
    np.testing.assert_allclose(float(n2.sum()), float(total), rtol=1e-6)
    for a, b in zip(fa, g2):
        assert torch.allclose(a.grad, b, rtol=1e-5, atol=1e-6 * float(a.grad.abs().max()))
    w = torch.tensor([0.5, 2.0, 0.0], device=dev())
    n3, g3 = ns_loss_and_grad(m, *fields, (wall, wall, None), weights=w, **kw)
    fb = [t.clone().requires_grad_(True) for t in fields]
    nb = ns_loss(m, *fb, (wall, wall, None), **kw)
    (0.5 * nb[0] + 2.0 * nb[1]).backward()
    for a, b in zip(fb, g3):
        assert torch.allclose(a.grad, b, rtol=1e-5, atol=1e-6 * float(a.grad.abs().max()))


def test_ns_launch_between_fsdt_defer_and_consumer_changes_nothing():
    from diffnet_amd import ops
    m = module(dict(domain_size=129, fem_basis_deg=2, ngp_1d=3))
    shape = (2, 1, 129, 129)
    flds = [cu(seeded(shape, 100 + i)) for i in range(3)]
    bcm = boundary_mask(shape).to(dev())
    consts = dict(D11=1.3, D12=0.4, D22=1.1, D66=0.6, A44=0.8, A55=0.9, q=1.2, wscale=0.3)
    wts = torch.tensor([1.0, 0.5, 2.0], device=dev())
    sm = module(dict(domain_size=129))
    sf = [cu(seeded(shape, 110 + i, -0.5)) for i in range(3)]

    def pair(interleave):
        Rs, _, h = ops.fsdt_apply(m.geom, *flds, bcm, want_sums=False, defer_norms=True, **consts)
        if interleave:
            ops.ns_apply(sm.geom, *sf, bcm, (0.1, 0.0, 0.0), 0.05, (0.2, 0.1), 0.25, want_norms=True)
        c = dict(consts, q=0.0)
        g, _, n = ops.fsdt_apply(m.geom, *Rs, bcm, want_sums=False, want_norms=True, in_num=wts, norms_from=h, **c)
        return g, n

    g0, n0 = pair(False)
    g1, n1 = pair(True)
    assert torch.equal(n0, n1) and torch.isfinite(n1).all()
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


def test_ns_and_stokes_interleaved_on_one_stream():
    from diffnet_amd import ops
    m = module(dict(domain_size=129))
    shape = (2, 1, 129, 129)
    f = [cu(seeded(shape, 120 + i, -0.5)) for i in range(3)]
    bcm = boundary_mask(shape).to(dev())

    def ns():
        return ops.ns_apply(m.geom, *f, bcm, (0.1, 0.0, 0.0), 0.05, (0.2, 0.1), 0.25, want_norms=True)

    def st():
        return ops.stokes_apply(m.geom, *f, bcm, (0.1, 0.0, 0.0), 0.7, 0.01, (0.2, 0.1), 0.25, want_norms=True)

    a_ns, a_st = ns(), st()
    seq = [ns(), st(), ns(), ns(), st(), st(), ns()]
    torch.cuda.synchronize()
    for i, r in enumerate(seq):
        ref = a_ns if i in (0, 2, 3, 6) else a_st
        for x, y in zip(r[0], ref[0]):
            assert torch.equal(x, y), i
        assert torch.equal(r[1], ref[1]) and torch.equal(r[2], ref[2]), i


def test_ns_loss_and_grad_graph_capture_replays_bitwise():
    from diffnet_amd.navier_stokes import ns_loss_and_grad
    m = rect_module(130, 47, 2)
    shape = (2, 1, 47, 130)
    fields = [cu(seeded(shape, 130 + i, -0.5)) for i in range(3)]
    wall = boundary_mask(shape).to(dev())
    kw = dict(bc_values=(cu(seeded((1, 1, 47, 130), 134, -0.5)), 0.0, 0.0), visco=0.05, f_gp=(0.3, cu(seeded((4, 46, 129), 135, -0.5))))
    bc = (wall, wall[:1].to(torch.uint8), None)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):                     # warm-up on the capture stream: workspace, prepared calls, default weights
            eager = ns_loss_and_grad(m, *fields, bc, **kw)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            static = ns_loss_and_grad(m, *fields, bc, **kw)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static[0], eager[0])
        for a, b in zip(static[1], eager[1]):
            assert torch.equal(a, b)
    with torch.no_grad():
        fields[0].mul_(0.5)                    # replays read the fields in place
    g.replay()
    again = ns_loss_and_grad(m, *fields, bc, **kw)
    torch.cuda.synchronize()
    assert torch.equal(static[0], again[0]) and not torch.equal(static[0], eager[0])


def test_ns_errors():
    from diffnet_amd import ops
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd.navier_stokes import ns_residuals
    m2 = module(dict(domain_size=17, fem_basis_deg=2))
    u = cu(seeded((1, 1, 17, 17), 1))
    with pytest.raises(DiffNetHipError):
        ns_residuals(m2, u, u, u, None)
    m = module(dict(domain_size=17))
    with pytest.raises(DiffNetHipError):
        ns_residuals(m, u.cpu(), u.cpu(), u.cpu(), None)
    with pytest.raises(DiffNetHipError):
        ns_residuals(m, u, u, u, boundary_mask((1, 1, 17, 17)))          # a CPU mask
    with pytest.raises(ValueError):
        ops.ns_apply(m.geom, u, u, u, in_num=u[0, 0, 0, :3].contiguous(), in_den=u[0, 0, 0, :3].contiguous())   # scaling without a VJP


def test_ns_ldc_example_fused_and_composed_agree():
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("ex_ns_ldc", os.path.join(here, "..", "examples", "ns_ldc.py"))
    ex = importlib.util.module_from_spec(spec)
    sys.modules["ex_ns_ldc"] = ex
    spec.loader.exec_module(ex)
    _, hf = ex.run(size=33, steps=15, stokes_steps=5, verbose=False, mode="fused")
    _, hc = ex.run(size=33, steps=15, stokes_steps=5, verbose=False, mode="composed")
    np.testing.assert_allclose(np.array(hf), np.array(hc), rtol=1e-3)
    assert hf[-1].sum() < hf[5].sum()
