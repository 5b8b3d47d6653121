#!/usr/bin/env python3
"""Golden vectors of the 2-D strong-form least-squares losses from the *imported* reference scripts.

Like tools/gen_golden_transport.py (whose approach and shims it reuses), this runs only where the reference repository is present.  It
imports the reference example scripts as modules and calls their own `loss` methods, unbound, on objects built by the library constructor,
on seeded random order-one u (no cancellation between the large second-derivative terms) with the scripts' own datasets.  Only data --
inputs and the reference's outputs -- is written, to tests/golden/loss_strongform_*.npz, batch 1.

  loss_strongform_burgers_n17.npz        examples/burgers/single_instance/01_2d_space_time.py, Burgers.loss: Q2, ngp 3, Burg2DXT(17)
  loss_strongform_poisson_q3_n10.npz     examples/poisson/single_instance/10_manufactured_strong_form_higher_order.py, Poisson.loss:
                                         Q3, ngp 3, RectangleManufactured(10)
  loss_strongform_poisson_q3_n10_g4.npz  the same at ngp 4

The scripts' `loss` returns only the scalar, so each file holds: kwargs, u, inputs (the dataset's channels as they are), forcing (the
nodal forcing tensor handed to `loss`), mask1 / mask2 (uint8: the two conditions as the script thresholds them), v1 (the value of
condition 1: a scalar or a field; condition 2 sets 0), coef = (ax, ay, b, dxx, dyy, fs), wscale, the reference's `loss` and its `grad`
with respect to u (autograd through the reference's own body).

Modules the scripts import that are absent on the machine (scipy, skimage) are stubbed here; nothing is installed.

Usage: python tools/gen_golden_strongform.py [--out tests/golden]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402
from gen_golden import T, install_shims, load_script, make, rng  # noqa: E402


def stub_missing(*names):
    for n in names:
        try:
            importlib.import_module(n)
        except ImportError:
            gen_golden.STUB_ROOTS.add(n)


def save(outdir, tag, kw, u, inputs, forcing, m1, m2, v1, coef, ref, grad):
    out = dict(kwargs=repr(kw), u=T(u), inputs=T(inputs), forcing=T(forcing), mask1=T(m1).astype(np.uint8), mask2=T(m2).astype(np.uint8),
               v1=np.asarray(v1, dtype=np.float32), coef=np.array(coef, dtype=np.float64), wscale=np.float64(1.0),
               loss=np.float32(T(ref)), grad=T(grad))
    np.savez_compressed(os.path.join(outdir, f"loss_strongform_{tag}.npz"), **out)
    print("strongform", tag, float(ref), float(grad.abs().max()))


def run(fn, m, u, inputs, frc):
    ur = u.clone().requires_grad_(True)
    ref = fn(m, ur, inputs, frc)
    grad, = torch.autograd.grad(ref, ur)
    return ref.detach(), grad


def gen(outdir):
    from DiffNet.DiffNetFEM import DiffNet2DFEM
    bur = load_script("examples/burgers/single_instance/01_2d_space_time.py", "ref_burgers_xt")
    s10 = load_script("examples/poisson/single_instance/10_manufactured_strong_form_higher_order.py", "ref_strong10")

    # ---- space-time Burgers: the script's own dataset (masks are the channels >= -5, condition 1 takes the field bc1_val)
    n = 17
    kw = dict(domain_size=n, fem_basis_deg=2)
    m = make(bur.Burgers, DiffNet2DFEM, **kw)
    inp, frc = bur.Burg2DXT(domain_size=n)[0]
    inputs, frc = inp[None].clone(), frc[None].clone()
    u = 2.0 * torch.rand((1, 1, n, n), generator=rng(91)) - 1.0
    ref, grad = run(bur.Burgers.loss, m, u, inputs, frc)
    save(outdir, "burgers_n17", kw, u, inputs, frc, inputs[:, 1:2] >= -5.0, inputs[:, 2:3] >= -5.0, T(inputs[0, 3]),
         (0.0, 1.0, 1.0, 0.0, 0.0, 0.0), ref, grad)

    # ---- strong-form Poisson on Q3 (masks are the channels > 0.5, condition 1 sets 1)
    n = 10
    for tag, ngp, seed in (("poisson_q3_n10", 3, 93), ("poisson_q3_n10_g4", 4, 95)):
        kw = dict(domain_size=n, fem_basis_deg=3) if ngp == 3 else dict(domain_size=n, fem_basis_deg=3, ngp_1d=ngp)
        m = make(s10.Poisson, DiffNet2DFEM, **kw)
        inp, frc = s10.RectangleManufactured(domain_size=n)[0]
        inputs, frc = inp[None].clone(), frc[None].clone()
        u = 2.0 * torch.rand((1, 1, n, n), generator=rng(seed)) - 1.0
        ref, grad = run(s10.Poisson.loss, m, u, inputs, frc)
        save(outdir, tag, kw, u, inputs, frc, inputs[:, 1:2] > 0.5, inputs[:, 2:3] > 0.5, 1.0, (0.0, 0.0, 0.0, 1.0, 1.0, 1.0), ref, grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    a = ap.parse_args()
    stub_missing("scipy", "skimage")
    install_shims()
    torch.manual_seed(0)
    gen(a.out)


if __name__ == "__main__":
    main()
