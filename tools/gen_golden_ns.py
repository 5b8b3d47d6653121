#!/usr/bin/env python3
"""Golden vectors of the 2-D Navier-Stokes (VMS) residual from the *imported* reference scripts.

Like tools/gen_golden_stokes.py (whose approach and shims it reuses), this runs only where the reference repository is present.  It
imports the reference example scripts as modules and calls their own `calc_residuals` / `loss` / `calc_residuals_ns` methods, unbound, on
objects built by the library constructor with the attributes those methods read set on seeded inputs.  Only data -- inputs and the
reference's outputs -- is written, to tests/golden/loss_ns_*.npz, batch 1 (the scripts' body broadcasts correctly at B = 1 only).  The
fields are order-one random values, so that the convective and stabilisation terms dominate the residuals.

  loss_ns_ldc_n17.npz      examples/navier-stokes/single_instance/e1_ns_ldc_resmin.py, NS_LDC: ngp 2, Re = 100, the lid profile
                           1 - 16 (x - 0.5)^4, walls on u / v, the corner pin on p, random forcing at the Gauss points
  loss_ns_ldc_n33_g3.npz   the same script at ngp 3, Re = 10, random boundary-value fields
  loss_ns_fps_rect.npz     e2_ns_fps_resmin.py, NS_FPS.calc_residuals_ns: 33 x 17 nodes on the unit square (hx != hy), Re = 20, no
                           forcing, an interior obstacle in the u / v masks

Each file: kwargs, the fields u, v, p, inputs (1, 5, ny, nx: x, y, bc1, bc2, bc3), f1 / f2 at the Gauss points (G, nely, nelx),
u_bc / v_bc / p_bc, visco / wscale / tau_h, R1..R3, norms and grad_norm{k} (3, 1, 1, ny, nx): the gradient of ||R_k|| wrt (u, v, p).

Usage: python tools/gen_golden_ns.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import T, boundary_mask, install_shims, load_script, make, rng  # noqa: E402
from gen_golden_stokes import coords, corner_pin  # noqa: E402


def run(outdir, tag, obj, body, loss, kw, inputs, fields, extra):
    """R = body(fields), norms = loss(fields) through the reference methods; the gradients of each norm wrt the three fields."""
    ur = tuple(t.clone().requires_grad_(True) for t in fields)
    R = body(obj, ur, inputs, torch.zeros_like(inputs[:, :1]))
    out = dict(kwargs=repr(kw), u=T(fields[0]), v=T(fields[1]), p=T(fields[2]), inputs=T(inputs),
               f1=T(obj.fx_gp).reshape(-1, *obj.fx_gp.shape[-2:]), f2=T(obj.fy_gp).reshape(-1, *obj.fy_gp.shape[-2:]),
               u_bc=T(obj.u_bc), v_bc=T(obj.v_bc), p_bc=T(obj.p_bc),
               R1=T(R[0]), R2=T(R[1]), R3=T(R[2]), **extra)
    if loss is None:
        norms = [torch.norm(r, "fro") for r in R]
    else:
        norms = loss(obj, ur, inputs, torch.zeros_like(inputs[:, :1]))
    out["norms"] = np.array([T(n) for n in norms])
    for i, nv in enumerate(norms):
        gs = torch.autograd.grad(nv, ur, retain_graph=True, allow_unused=True)
        out[f"grad_norm{i + 1}"] = np.stack([T(torch.zeros_like(f) if x is None else x) for x, f in zip(gs, fields)], 0)
    np.savez_compressed(os.path.join(outdir, f"loss_ns_{tag}.npz"), **out)
    print("ns", tag, out["norms"])


def gen(outdir):
    from DiffNet.DiffNetFEM import DiffNet2DFEM
    ldc = load_script("examples/navier-stokes/single_instance/e1_ns_ldc_resmin.py", "ref_ns_ldc")
    fps = load_script("examples/navier-stokes/single_instance/e2_ns_fps_resmin.py", "ref_ns_fps")

    # ---- lid-driven cavity, ngp 2 (e1_ns_ldc_resmin.py:97-132 sets these attributes in __init__)
    for tag, n, ngp, Re, seed, value_fields in (("ldc_n17", 17, 2, 100.0, 51, False), ("ldc_n33_g3", 33, 3, 10.0, 53, True)):
        kw = dict(domain_size=n) if ngp == 2 else dict(domain_size=n, ngp_1d=ngp)
        m = make(ldc.NS_LDC, DiffNet2DFEM, **kw)
        g = rng(seed)
        m.Re, m.viscosity = Re, 1.0 / Re
        xx, yy = coords(m, n, n)
        m.fx_gp = torch.rand(m.xgp.shape, generator=g) - 0.5
        m.fy_gp = torch.rand(m.xgp.shape, generator=g) - 0.5
        if value_fields:
            m.u_bc, m.v_bc, m.p_bc = (2.0 * torch.rand((n, n), generator=g) - 1.0 for _ in range(3))
        else:
            u_bc = torch.zeros(n, n)
            u_bc[-1, :] = 1.0 - 16.0 * (xx[-1, :] - 0.5) ** 4
            m.u_bc, m.v_bc, m.p_bc = u_bc, torch.zeros(n, n), torch.zeros(n, n)
        walls = boundary_mask((1, 1, n, n))
        inputs = torch.cat([xx[None, None], yy[None, None], walls, walls, corner_pin((1, 1, n, n))], 1)
        fields = tuple(2.0 * torch.rand((1, 1, n, n), generator=g) - 1.0 for _ in range(3))
        run(outdir, tag, m, ldc.NS_LDC.calc_residuals, ldc.NS_LDC.loss, kw, inputs, fields,
            dict(visco=m.viscosity, wscale=(0.5 * m.h) ** 2, tau_h=np.array([m.h, m.h])))

    # ---- flow past a square, the nonlinear stage on a rectangular-element mesh (trnsfrm_jac = (hx/2)(hy/2), no forcing)
    kw = dict(domain_sizes=(33, 17), domain_lengths=(1.0, 1.0), domain_size=33, domain_length=1.0)
    m = make(fps.NS_FPS, DiffNet2DFEM, **kw)
    ny, nx, Re = m.domain_sizeY, m.domain_sizeX, 20.0
    g = rng(57)
    m.Re, m.viscosity = Re, 1.0 / Re
    xx, yy = coords(m, ny, nx)
    m.fx_gp = torch.zeros(m.xgp.shape)
    m.fy_gp = torch.zeros(m.xgp.shape)
    u_bc = torch.zeros(ny, nx)
    u_bc[:, 0] = 1.0 - (2.0 * yy[:, 0] / m.domain_lengthY - 1.0) ** 2
    u_bc[0, :] = 0.0
    u_bc[-1, :] = 0.0
    m.u_bc, m.v_bc, m.p_bc = u_bc, torch.zeros(ny, nx), torch.zeros(ny, nx)
    wall = torch.zeros((1, 1, ny, nx))
    wall[..., 0, :] = 1.0
    wall[..., -1, :] = 1.0
    wall[..., :, 0] = 1.0
    wall[..., 6:11, 8:13] = 1.0                      # the obstacle
    outlet = torch.zeros((1, 1, ny, nx))
    outlet[..., :, -1] = 1.0
    inputs = torch.cat([xx[None, None], yy[None, None], wall, wall, outlet], 1)
    fields = tuple(2.0 * torch.rand((1, 1, ny, nx), generator=g) - 1.0 for _ in range(3))
    run(outdir, "fps_rect", m, fps.NS_FPS.calc_residuals_ns, None, kw, inputs, fields,
        dict(visco=m.viscosity, wscale=(0.5 * m.hx) * (0.5 * m.hy), tau_h=np.array([m.hx, m.hy])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    a = ap.parse_args()
    install_shims()
    torch.manual_seed(0)
    gen(a.out)


if __name__ == "__main__":
    main()
