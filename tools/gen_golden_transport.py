#!/usr/bin/env python3
"""Golden vectors of the 2-D scalar transport (SUPG) residual loss from the *imported* reference scripts.

Like tools/gen_golden_ns.py (whose approach and shims it reuses), this runs only where the reference repository is present.  It imports
the reference example scripts as modules and calls their own `loss` methods, unbound, on objects built by the library constructor with the
attributes those methods read set on seeded inputs.  Only data -- inputs and the reference's outputs -- is written, to
tests/golden/loss_transport_*.npz, batch 1, random order-one u, random Gauss-point forcing in (-20, 20) (the size of a . grad u there, so
that the forcing is visible in the loss and its gradient).

  loss_transport_advdiff_n17.npz       examples/poisson/single_instance/e17_adv_diff_2d_resmin.py, AdvDiff2d.loss: ngp 2, random nu,
                                       random forcing at the Gauss points, diffusivity 1e-2 with tau recomputed (diffusion visible in fp32)
  loss_transport_stheat_n33_g3.npz     e3_st_mms_resmin.py, SpaceTimeHeat.loss_resmin: ngp 3; the dataset's two masks overlap in the corners
                                       of the first row where its own u0 is ~0, so the method is handed a dataset object whose u0 is a seeded
                                       random field -- only then does the file pin which condition wins on the rows of R
  loss_transport_allencahn_n17.npz     e18_allen_cahn_ice_melt.py, AllenCahnIceMelt.loss: ngp 2, the cubic reaction
  loss_transport_allencahn_n9_g4.npz   the same at ngp 4

The scripts' `loss` returns only the scalar, so each file holds: kwargs, u, inputs (1, 3, ny, nx: nu, bc1, bc2), f_gp (G, nely, nelx),
v1 (the value of condition 1: a scalar or the field u0), adv / kappa / tau / react / wscale / r_first_wins, uses_nu (only e17 reads
the nu channel of its inputs), the reference's `loss` and its
`grad` with respect to u (autograd through the reference's own body).

Usage: python tools/gen_golden_transport.py [--out tests/golden]
"""
import argparse
import math
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import T, install_shims, load_script, make, rng  # noqa: E402


def save(outdir, tag, kw, u, inputs, m, v1, coef, first, ref, grad, uses_nu=False):
    adv, kappa, tau, react = coef
    f = T(m.f_gp)
    out = dict(kwargs=repr(kw), u=T(u), inputs=T(inputs), f_gp=f.reshape(-1, *f.shape[-2:]), v1=np.asarray(v1, dtype=np.float32),
               adv=np.array(adv, dtype=np.float64), kappa=np.array(kappa, dtype=np.float64), tau=np.float64(tau),
               react=np.array(react, dtype=np.float64), uses_nu=np.int32(uses_nu), wscale=np.float64((0.5 * m.h) ** 2), r_first_wins=np.int32(first),
               loss=np.float32(T(ref)), grad=T(grad))
    np.savez_compressed(os.path.join(outdir, f"loss_transport_{tag}.npz"), **out)
    print("transport", tag, float(ref), float(grad.abs().max()))


def gen(outdir):
    from DiffNet.DiffNetFEM import DiffNet2DFEM
    from DiffNet.datasets.single_instances import rectangles as R
    e17 = load_script("examples/poisson/single_instance/e17_adv_diff_2d_resmin.py", "ref_e17")
    e3 = load_script("examples/poisson/single_instance/e3_st_mms_resmin.py", "ref_e3")
    e18 = load_script("examples/poisson/single_instance/e18_allen_cahn_ice_melt.py", "ref_e18")

    def setup(cls, n, ngp, seed):
        kw = dict(domain_size=n) if ngp == 2 else dict(domain_size=n, ngp_1d=ngp)
        m = make(cls, DiffNet2DFEM, **kw)
        g = rng(seed)
        u = 2.0 * torch.rand((1, 1, n, n), generator=g) - 1.0
        m.f_gp = 40.0 * (torch.rand(m.xgp.shape, generator=g) - 0.5)     # as large as a . grad u of an order-one u on these meshes
        return kw, m, g, u

    def run(fn, m, u, inputs, frc):
        ur = u.clone().requires_grad_(True)
        ref = fn(m, ur, inputs, frc)
        ref = ref[0] if isinstance(ref, tuple) else ref
        grad, = torch.autograd.grad(ref, ur)
        return ref.detach(), grad

    # ---- e17: steady advection-diffusion (e17_adv_diff_2d_resmin.py:30-45 sets these attributes in __init__)
    n = 17
    kw, m, g, u = setup(e17.AdvDiff2d, n, 2, 71)
    ds = R.AdvDiff2dRectangle(domain_size=n)
    m.dataset = ds
    m.adv = np.array([math.cos(math.pi / 6), math.sin(math.pi / 6)])
    m.diffusivity = 1e-2
    m.tau = 1.0 / (2.0 / m.h + 4.0 * m.diffusivity / m.h ** 2)
    inp, frc = ds[0]
    inputs = inp[None].clone()
    inputs[:, 0:1] = 0.5 + torch.rand((1, 1, n, n), generator=g)
    ref, grad = run(e17.AdvDiff2d.loss, m, u, inputs, frc[None])
    save(outdir, "advdiff_n17", kw, u, inputs, m, 1.0, (m.adv, (m.diffusivity, m.diffusivity), m.tau, (0, 0, 0, 0)), 0, ref, grad, uses_nu=True)

    # ---- e3: space-time heat, ngp 3, a random u0 on the dataset object the method reads
    n = 33
    kw, m, g, u = setup(e3.SpaceTimeHeat, n, 3, 73)
    ds = R.SpaceTimeRectangleManufactured(domain_size=n)
    inp, frc = ds[0]
    u0 = 2.0 * torch.rand((n, n), generator=g) - 1.0
    m.dataset = types.SimpleNamespace(u0=u0)
    m.diffusivity = ds.diffusivity
    m.tau = 1.0 / (2.0 / m.h)
    inputs = inp[None].clone()
    ref, grad = run(e3.SpaceTimeHeat.loss_resmin, m, u, inputs, frc[None])
    save(outdir, "stheat_n33_g3", kw, u, inputs, m, T(u0), ((0.0, 1.0), (m.diffusivity, 0.0), m.tau, (0, 0, 0, 0)), 1, ref, grad)

    # ---- e18: space-time Allen-Cahn, ngp 2 and ngp 4
    for tag, n, ngp, seed in (("allencahn_n17", 17, 2, 75), ("allencahn_n9_g4", 9, 4, 77)):
        kw, m, g, u = setup(e18.AllenCahnIceMelt, n, ngp, seed)
        ds = R.AllenCahnIceMeltRectangle(domain_size=n)
        m.dataset = ds
        m.ac_A, m.ac_Cn, m.ac_D, m.ac_k = ds.ac_A, ds.ac_Cn, ds.ac_D, ds.ac_k
        inp, frc = ds[0]
        inputs = inp[None].clone()
        ref, grad = run(e18.AllenCahnIceMelt.loss, m, u, inputs, frc[None])
        D, A, k, Cn = (float(x) for x in (m.ac_D, m.ac_A, m.ac_k, m.ac_Cn))
        save(outdir, tag, kw, u, inputs, m, T(ds.u0),
             ((0.0, 1.0), (D * Cn ** 2, D * Cn ** 2), 0.0, (-D * D * k, 2 * D * D * A, -6 * D * D * A, 4 * D * D * A)), 0, ref, grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    a = ap.parse_args()
    install_shims()
    torch.manual_seed(0)
    gen(a.out)


if __name__ == "__main__":
    main()
