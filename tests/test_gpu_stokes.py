"""GPU tests of the fused 2-D Stokes (PSPG) residual (dn_stokes_apply, csrc/stokes.hip; diffnet_amd/stokes.py): against the reference
fixtures (tests/golden/loss_stokes_*.npz, the reference scripts' own residual bodies), against the same residuals composed from the
drop-in operators on every mask / value / forcing form, the adjoint identity of the transpose launch, batch independence, the in-kernel
norms, isolation of its reduction workspace from a deferred FSDT pair, the errors, and the lid-driven-cavity example."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import boundary_mask, close, cu, dev, load, module, seeded

pytestmark = pytest.mark.gpu

FIXTURES = ["ldc_n17", "mms_n33_g3", "fps_rect"]


def fixture_inputs(z):
    m = module(eval(str(z["kwargs"])))
    inp = cu(z["inputs"])
    bc = tuple(inp[:, 2 + k:3 + k].contiguous() for k in range(3))
    vals = tuple(cu(z[n]).reshape(1, 1, *z[n].shape) for n in ("u_bc", "v_bc", "p_bc"))
    f_gp = (cu(z["f1"]), cu(z["f2"])) if np.abs(z["f1"]).max() > 0 or np.abs(z["f2"]).max() > 0 else None
    kw = dict(bc_values=vals, visco=float(z["visco"]), pspg=float(z["pspg"]), f_gp=f_gp, wscale=float(z["wscale"]))
    return m, bc, kw


@pytest.mark.parametrize("tag", FIXTURES)
def test_stokes_vs_reference_golden(tag):
    from diffnet_amd.stokes import stokes_loss, stokes_residuals
    z = load(f"loss_stokes_{tag}.npz")
    m, bc, kw = fixture_inputs(z)
    fields = [cu(z[n]).requires_grad_(True) for n in ("u", "v", "p")]
    Rs = stokes_residuals(m, *fields, bc, **kw)
    for i, R in enumerate(Rs):
        close(R, z[f"R{i + 1}"], rtol=1e-4, arel=1e-5, msg=f"R{i + 1}")
    norms = stokes_loss(m, *fields, bc, **kw)
    for i, nv in enumerate(norms):
        np.testing.assert_allclose(float(nv), float(z["norms"][i]), rtol=1e-4)
        gs = torch.autograd.grad(nv, fields, retain_graph=True)
        ref = z[f"grad_norm{i + 1}"]
        for q, (gq, rq) in enumerate(zip(gs, ref)):
            close(gq, rq, rtol=1e-4, arel=1e-5 * float(np.abs(ref).max()) / max(float(np.abs(rq).max()), 1e-30), msg=f"grad {i} {q}")


def rect_module(nx, ny, ngp, lengths=(1.0, 0.7)):
    return module(dict(domain_sizes=(nx, ny), domain_lengths=lengths, domain_size=nx, domain_length=lengths[0], ngp_1d=ngp))


def compare(m, fields, bc, kw, rtol=2e-5, msg=""):
    from diffnet_amd.stokes import stokes_residuals, stokes_residuals_composed
    got = stokes_residuals(m, *fields, bc, **kw)
    ref = stokes_residuals_composed(m, *fields, bc, **kw)
    for k in range(3):
        scale = float(ref[k].abs().max())
        err = float((got[k] - ref[k]).abs().max())
        assert err <= rtol * max(scale, 1e-30), f"{msg} R{k + 1}: {err} vs max {scale}"


# mask forms: fp32 / u8 / bool, shared / per sample, a None entry; value fields (shared / per sample) and constants; forcing none / constant /
# Gauss-point tensors shared and batched
@pytest.mark.parametrize("nx,ny,B,ngp", [(65, 65, 2, 2), (257, 257, 3, 2), (130, 47, 2, 3), (33, 129, 3, 4), (64, 5, 1, 3), (2, 2, 2, 2),
                                         (125, 3, 2, 4)])
def test_stokes_fused_matches_composed(nx, ny, B, ngp):
    m = rect_module(nx, ny, ngp)
    shape = (B, 1, ny, nx)
    fields = [cu(seeded(shape, 10 + i, -0.5)) for i in range(3)]
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(3)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float())
    shared = wall[:1].contiguous()
    G, eshape = ngp * ngp, (ny - 1, nx - 1)
    f_sh = cu(seeded((G, *eshape), 20, -0.5))
    f_b = cu(seeded((B, G, *eshape), 21, -0.5))
    vfield = cu(seeded(shape, 30, -0.5))
    vshared = cu(seeded((1, 1, ny, nx), 31, -0.5))
    cases = [
        ("fp32 shared, constants, no forcing", shared, (0.3, -0.2, 0.1), None),
        ("fp32 per sample, value fields, gp forcing shared", (wall, blob, shared), (vfield, vshared, 0.5), (f_sh, f_sh)),
        ("u8 per sample, None entry, batched forcing", (blob.to(torch.uint8), None, shared.to(torch.uint8)), (vshared, 0.0, vfield), (f_b, None)),
        ("bool, constant forcing", (wall.bool(), wall.bool(), blob.bool()), (0.0, 1.0, vshared), (0.7, -1.3)),
        ("no masks, mixed forcing", None, (0.0, 0.0, 0.0), (-0.4, f_b)),
    ]
    for name, bc, vals, f in cases:
        kw = dict(bc_values=vals, visco=0.8, pspg=0.03, f_gp=f, wscale=None)
        compare(m, fields, bc, kw, msg=name)


def _dot(a, b):
    return sum(float((x.double() * y.double()).sum()) for x, y in zip(a, b))


@pytest.mark.parametrize("ngp", [2, 3, 4])
def test_stokes_transpose_launch_is_the_adjoint(ngp):
    from diffnet_amd import ops
    from diffnet_amd.stokes import stokes_loss, stokes_residuals_composed
    m = rect_module(70, 41, ngp)
    B = 2
    shape = (B, 1, 41, 70)
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(8)
    bc = (wall, cu((torch.rand(shape, generator=rs) < 0.3).float()), wall[:1].to(torch.uint8))
    x = [cu(seeded(shape, 40 + i, -0.5)) for i in range(3)]
    y = [cu(seeded(shape, 50 + i, -0.5)) for i in range(3)]
    lin = dict(bc_values=(0.0, 0.0, 0.0), visco=1.3, pspg=0.02, f_gp=None, wscale=0.3)
    Jx, _ = ops.stokes_apply(m.geom, *x, bc, want_sums=False, **lin)
    JTy, _ = ops.stokes_apply(m.geom, *y, bc, want_sums=False, transpose=True, **lin)
    lhs, rhs = _dot(Jx, y), _dot(x, JTy)
    assert abs(lhs - rhs) <= 2e-5 * (abs(lhs) + abs(rhs)), (lhs, rhs)
    # autograd of the three norms against autograd through the composition (with forcing and value fields: they drop out of the VJP)
    kw = dict(bc_values=(cu(seeded(shape, 60, -0.5)), 0.4, 0.0), visco=1.3, pspg=0.02, f_gp=(0.5, cu(seeded((ngp * ngp, 40, 69), 61))), wscale=0.3)
    fa = [t.clone().requires_grad_(True) for t in x]
    fb = [t.clone().requires_grad_(True) for t in x]
    na = stokes_loss(m, *fa, bc, **kw)
    nb = [torch.norm(R) for R in stokes_residuals_composed(m, *fb, bc, **kw)]
    for k in range(3):
        np.testing.assert_allclose(float(na[k]), float(nb[k]), rtol=2e-5)
        ga = torch.autograd.grad(na[k], fa, retain_graph=True)
        gb = torch.autograd.grad(nb[k], fb, retain_graph=True, allow_unused=True)
        for q in range(3):
            ref = torch.zeros_like(ga[q]) if gb[q] is None else gb[q]
            scale = max(float(ref.abs().max()), float(ga[q].abs().max()), 1e-30)
            assert float((ga[q] - ref).abs().max()) <= 1e-4 * scale, (k, q)


def test_stokes_batch_samples_are_independent_bitwise():
    from diffnet_amd import ops
    m = rect_module(257, 129, 3)
    B = 3
    shape = (B, 1, 129, 257)
    fields = [cu(seeded(shape, 70 + i, -0.5)) for i in range(3)]
    wall = boundary_mask(shape).to(dev())
    rs = torch.Generator().manual_seed(9)
    blob = cu((torch.rand(shape, generator=rs) < 0.2).float())
    vals = (cu(seeded(shape, 80, -0.5)), 0.2, 0.0)
    f = (cu(seeded((B, 9, 128, 256), 81, -0.5)), 0.3)
    kw = dict(visco=0.5, pspg=0.01, wscale=0.2)
    outs, _, norms = ops.stokes_apply(m.geom, *fields, (wall, blob, blob.to(torch.uint8)), vals, f_gp=f, want_norms=True, **kw)
    for b in range(B):
        sl = slice(b, b + 1)
        ob, _ = ops.stokes_apply(m.geom, *[t[sl].contiguous() for t in fields], (wall[sl].contiguous(), blob[sl].contiguous(), blob[sl].to(torch.uint8)),
                                 (vals[0][sl].contiguous(), 0.2, 0.0), f_gp=(f[0][sl].contiguous(), 0.3), want_sums=False, **kw)
        for k in range(3):
            assert torch.equal(outs[k][sl], ob[k]), (b, k)


def test_stokes_norms_zero_residual_and_loss_and_grad():
    from diffnet_amd import ops
    from diffnet_amd.stokes import stokes_loss, stokes_loss_and_grad, stokes_total_loss
    m = rect_module(97, 65, 2)
    B = 2
    shape = (B, 1, 65, 97)
    fields = [cu(seeded(shape, 90 + i, -0.5)) for i in range(3)]
    wall = boundary_mask(shape).to(dev())
    kw = dict(bc_values=(0.1, 0.0, 0.0), visco=1.0, pspg=0.02, f_gp=(0.3, -0.2), wscale=None)
    outs, sums, norms = ops.stokes_apply(m.geom, *fields, wall[:1].contiguous(), kw["bc_values"], kw["visco"], kw["pspg"], kw["f_gp"],
                                         (0.5 * m.hx) * (0.5 * m.hy), want_norms=True)
    ref = np.array([float((o.double() ** 2).sum()) for o in outs])
    np.testing.assert_allclose(sums.cpu().numpy(), ref, rtol=1e-6)          # (per-lane partial sums are fp32, the rest fp64)
    np.testing.assert_allclose(norms.cpu().numpy(), np.sqrt(ref), rtol=1e-6)
    # every node Dirichlet with zero values: zero residuals, zero norms, zero (not NaN) gradients
    ones = torch.ones((1, 1, 65, 97), device=dev())
    fz = [t.clone().requires_grad_(True) for t in fields]
    nz = stokes_loss(m, *fz, ones)
    assert all(float(x) == 0.0 for x in nz)
    g = torch.autograd.grad(sum(nz), fz)
    assert all(torch.isfinite(t).all() and float(t.abs().max()) == 0.0 for t in g)
    # stokes_loss_and_grad == autograd of stokes_total_loss (and weights)
    fa = [t.clone().requires_grad_(True) for t in fields]
    total = stokes_total_loss(m, *fa, (wall, wall, None), **kw)
    total.backward()
    n2, g2 = stokes_loss_and_grad(m, *fields, (wall, wall, None), **kw)
    np.testing.assert_allclose(float(n2.sum()), float(total), rtol=1e-6)
    for a, b in zip(fa, g2):
        assert torch.allclose(a.grad, b, rtol=1e-5, atol=1e-6 * float(a.grad.abs().max()))
    w = torch.tensor([0.5, 2.0, 0.0], device=dev())
    n3, g3 = stokes_loss_and_grad(m, *fields, (wall, wall, None), weights=w, **kw)
    fb = [t.clone().requires_grad_(True) for t in fields]
    nb = stokes_loss(m, *fb, (wall, wall, None), **kw)
    (0.5 * nb[0] + 2.0 * nb[1]).backward()
    for a, b in zip(fb, g3):
        assert torch.allclose(a.grad, b, rtol=1e-5, atol=1e-6 * float(a.grad.abs().max()))


def test_stokes_launch_between_fsdt_defer_and_consumer_changes_nothing():
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
            ops.stokes_apply(sm.geom, *sf, bcm, (0.1, 0.0, 0.0), 0.7, 0.01, (0.2, 0.1), 0.25, want_norms=True)
        c = dict(consts, q=0.0)
        g, _, n = ops.fsdt_apply(m.geom, *Rs, bcm, want_sums=False, want_norms=True, in_num=wts, norms_from=h, **c)
        return g, n

    g0, n0 = pair(False)
    g1, n1 = pair(True)
    assert torch.equal(n0, n1) and torch.isfinite(n1).all()
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


def test_stokes_errors():
    from diffnet_amd import ops
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd.stokes import stokes_residuals
    m2 = module(dict(domain_size=17, fem_basis_deg=2))
    u = cu(seeded((1, 1, 17, 17), 1))
    with pytest.raises(DiffNetHipError):
        stokes_residuals(m2, u, u, u, None)
    m3 = module(dict(domain_size=9, nsd=3))
    u3 = cu(seeded((1, 1, 9, 9, 9), 1))
    with pytest.raises(DiffNetHipError):
        ops.stokes_apply(m3.geom, u3, u3, u3)
    m = module(dict(domain_size=17))
    with pytest.raises(DiffNetHipError):
        stokes_residuals(m, u.cpu(), u.cpu(), u.cpu(), None)
    with pytest.raises(DiffNetHipError):
        stokes_residuals(m, u, u, u, boundary_mask((1, 1, 17, 17)))          # a CPU mask


def test_stokes_ldc_example_fused_and_composed_agree():
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("ex_stokes_ldc", os.path.join(here, "..", "examples", "stokes_ldc.py"))
    ex = importlib.util.module_from_spec(spec)
    sys.modules["ex_stokes_ldc"] = ex
    spec.loader.exec_module(ex)
    _, hf = ex.run(size=33, steps=20, verbose=False, mode="fused")
    _, hc = ex.run(size=33, steps=20, verbose=False, mode="composed")
    np.testing.assert_allclose(np.array(hf), np.array(hc), rtol=1e-4)
    assert hf[-1].sum() < hf[0].sum()
