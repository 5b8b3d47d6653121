#!/usr/bin/env python3
"""Golden vectors of the 2-D Stokes (PSPG) residual from the *imported* reference scripts.

Like tools/gen_golden.py (whose shims and helpers it reuses; that file is left as it is), this runs only where the reference
repository is present.  It imports the reference example scripts as modules and calls their own `calc_residuals` / `loss` /
`calc_residuals_stokes` methods, unbound, on objects built by the library constructor with the attributes those methods read set
on seeded inputs.  Only data -- inputs and the reference's outputs -- is written, to tests/golden/loss_stokes_*.npz, batch 1 (the
scripts' body broadcasts correctly at B = 1 only).

  loss_stokes_ldc_n17.npz     examples/stokes/single_instance/e2_stokes_ldc_resmin.py, Stokes_LDC: ngp 2, Re = 10, the lid profile
                              1 - 16 (x - 0.5)^4, walls on u / v, the corner pin on p, random forcing at the Gauss points
  loss_stokes_mms_n33_g3.npz  e1_stokes_mms_resmin_loss2.py, Stokes_LDC: ngp 3, Re = 2, random boundary-value fields
  loss_stokes_fps_rect.npz    navier-stokes/single_instance/e2_ns_fps_resmin.py, NS_FPS.calc_residuals_stokes: 33 x 17 nodes on the
                              unit square (hx != hy), J = 1, no forcing, an interior obstacle in the u / v masks

Each file: kwargs, the fields u, v, p, inputs (1, 5, ny, nx: x, y, bc1, bc2, bc3), f1 / f2 at the Gauss points (G, nely, nelx),
u_bc / v_bc / p_bc, visco / pspg / wscale, R1..R3, norms and grad_norm{k} (3, 1, 1, ny, nx): the gradient of ||R_k|| wrt (u, v, p).

Usage: python tools/gen_golden_stokes.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import T, boundary_mask, install_shims, load_script, make, rng  # noqa: E402


def corner_pin(shape):
    m = torch.zeros(shape)
    m[..., 0, 0] = 1.0
    return m


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
        gs = torch.autograd.grad(nv, ur, retain_graph=True, allow_unused=True)         # (||R1|| does not depend on v, ||R2|| on u)
        out[f"grad_norm{i + 1}"] = np.stack([T(torch.zeros_like(f) if x is None else x) for x, f in zip(gs, fields)], 0)
    np.savez_compressed(os.path.join(outdir, f"loss_stokes_{tag}.npz"), **out)
    print("stokes", tag, out["norms"])


def coords(obj, n_y, n_x):
    x = torch.linspace(0, obj.domain_lengthX, n_x)
    y = torch.linspace(0, obj.domain_lengthY, n_y)
    yy, xx = torch.meshgrid(y, x, indexing="ij")
    return xx, yy


def gen(outdir):
    from DiffNet.DiffNetFEM import DiffNet2DFEM
    ldc = load_script("examples/stokes/single_instance/e2_stokes_ldc_resmin.py", "ref_stokes_ldc")
    mms2 = load_script("examples/stokes/single_instance/e1_stokes_mms_resmin_loss2.py", "ref_stokes_mms_loss2")
    fps = load_script("examples/navier-stokes/single_instance/e2_ns_fps_resmin.py", "ref_ns_fps")

    # ---- lid-driven cavity, ngp 2 (e2_stokes_ldc_resmin.py:100-130 sets these attributes in __init__)
    kw = dict(domain_size=17)
    m = make(ldc.Stokes_LDC, DiffNet2DFEM, **kw)
    n, Re = m.domain_size, 10.0
    g = rng(41)
    m.Re, m.viscosity, m.pspg_param = Re, 1.0 / Re, m.h ** 2 * Re / 12.0
    xx, yy = coords(m, n, n)
    m.fx_gp = torch.rand(m.xgp.shape, generator=g) - 0.5
    m.fy_gp = torch.rand(m.xgp.shape, generator=g) - 0.5
    u_bc = torch.zeros(n, n)
    u_bc[-1, :] = 1.0 - 16.0 * (xx[-1, :] - 0.5) ** 4
    m.u_bc, m.v_bc, m.p_bc = u_bc, torch.zeros(n, n), torch.zeros(n, n)
    walls = boundary_mask((1, 1, n, n))
    inputs = torch.cat([xx[None, None], yy[None, None], walls, walls, corner_pin((1, 1, n, n))], 1)
    fields = tuple(torch.rand((1, 1, n, n), generator=g) - 0.5 for _ in range(3))
    run(outdir, "ldc_n17", m, ldc.Stokes_LDC.calc_residuals, ldc.Stokes_LDC.loss, kw, inputs, fields,
        dict(visco=m.viscosity, pspg=m.pspg_param, wscale=(0.5 * m.h) ** 2))

    # ---- manufactured-solution script (loss2 form), ngp 3, nonzero boundary-value fields
    kw = dict(domain_size=33, ngp_1d=3)
    m = make(mms2.Stokes_LDC, DiffNet2DFEM, **kw)
    n, Re = m.domain_size, 2.0
    g = rng(43)
    m.Re, m.viscosity, m.pspg_param = Re, 1.0 / Re, m.h ** 2 * Re / 12.0
    xx, yy = coords(m, n, n)
    m.fx_gp = torch.rand(m.xgp.shape, generator=g) - 0.5
    m.fy_gp = torch.rand(m.xgp.shape, generator=g) - 0.5
    m.u_bc, m.v_bc, m.p_bc = (torch.rand((n, n), generator=g) - 0.5 for _ in range(3))
    walls = boundary_mask((1, 1, n, n))
    pmask = corner_pin((1, 1, n, n))
    pmask[..., -1, -1] = 1.0
    inputs = torch.cat([xx[None, None], yy[None, None], walls, walls, pmask], 1)
    fields = tuple(torch.rand((1, 1, n, n), generator=g) - 0.5 for _ in range(3))
    run(outdir, "mms_n33_g3", m, mms2.Stokes_LDC.calc_residuals, mms2.Stokes_LDC.loss, kw, inputs, fields,
        dict(visco=m.viscosity, pspg=m.pspg_param, wscale=(0.5 * m.h) ** 2))

    # ---- flow past a square: the Stokes stage of the Navier-Stokes script on a rectangular-element mesh (J = 1, no forcing)
    kw = dict(domain_sizes=(33, 17), domain_lengths=(1.0, 1.0), domain_size=33, domain_length=1.0)
    m = make(fps.NS_FPS, DiffNet2DFEM, **kw)
    ny, nx, Re = m.domain_sizeY, m.domain_sizeX, 5.0
    g = rng(47)
    m.Re, m.viscosity, m.pspg_param = Re, 1.0 / Re, m.hx * m.hy * Re / 12.0
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
    fields = tuple(torch.rand((1, 1, ny, nx), generator=g) - 0.5 for _ in range(3))
    run(outdir, "fps_rect", m, fps.NS_FPS.calc_residuals_stokes, None, kw, inputs, fields,
        dict(visco=m.viscosity, pspg=m.pspg_param, wscale=1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    a = ap.parse_args()
    install_shims()
    torch.manual_seed(0)
    gen(a.out)


if __name__ == "__main__":
    main()
