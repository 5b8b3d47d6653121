#!/usr/bin/env python3
"""Golden vectors of the topology-optimisation losses from the *imported* reference script.

Like tools/gen_golden_transport.py (whose approach and shims it reuses), this runs only where the reference repository is present.  It
imports examples/poisson/single_instance/16_topopt.py as a module and calls `Poisson.loss` and `Poisson.compliance`, unbound, on an object
built by the library constructor, on seeded inputs.  Only data -- inputs and the reference's outputs -- is written:

  loss_topopt_n17.npz, loss_topopt_n33.npz   batch 1, ngp 2: random order-one u, random raw coefficient input rho (the script forms
                                             nu = 0.001 + sigmoid(rho)^3 itself), random forcing in (0.5, 1.5), bc1 on part of the last row,
                                             bc2 on the first row and column (the script's own dataset has an empty bc1)

Each file holds: kwargs, u, rho, inputs (1, 4, n, n: bc1, bc2, xx, yy), f, the reference's `loss` with its autograd gradients `loss_du`,
`loss_drho`, its `compliance` with `compliance_du`, `compliance_drho` (zero: the method does not read the coefficient), and -- because
`loss` adds the two Dirichlet penalty terms to every element -- their value `dbc` and gradient `dbc_du` separately, so that a test can
subtract them.  `loss` applies no Dirichlet substitution (the penalties stand in for it); `compliance` does.

Usage: python tools/gen_golden_topopt.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import T, install_shims, load_script, make, rng  # noqa: E402


def gen(outdir):
    from DiffNet.DiffNetFEM import DiffNet2DFEM
    ts = load_script("examples/poisson/single_instance/16_topopt.py", "ref_topopt")
    for n, seed in ((17, 81), (33, 83)):
        kw = dict(domain_size=n)
        m = make(ts.Poisson, DiffNet2DFEM, **kw)
        m.median_filter = ts.MedianPool2d(kernel_size=3, padding=1)        # Poisson.__init__ sets it (the filter is the identity)
        g = rng(seed)
        u = 2.0 * torch.rand((1, 1, n, n), generator=g) - 1.0
        rho = 4.0 * torch.rand((1, 1, n, n), generator=g) - 2.0
        f = 0.5 + torch.rand((1, 1, n, n), generator=g)
        inp, _ = ts.Rectangle(domain_size=n)[0]
        inputs = inp[None].clone()
        inputs[0, 0, -1, n // 3:(2 * n) // 3] = 1.0

        def run(fn):
            ur, rr = u.clone().requires_grad_(True), rho.clone().requires_grad_(True)
            val = fn(m, [ur, rr], inputs, f)
            gu, gr = torch.autograd.grad(val, (ur, rr), allow_unused=True)
            return val.detach(), gu, (torch.zeros_like(rho) if gr is None else gr)

        loss, lu, lr = run(ts.Poisson.loss)
        comp, cu, cr = run(ts.Poisson.compliance)
        # the penalty terms of `loss` alone: the difference between the method on the given masks and on empty ones
        blank = inputs.clone()
        blank[:, 0:2] = 0.0
        ur = u.clone().requires_grad_(True)
        pen = ts.Poisson.loss(m, [ur, rho], inputs, f) - ts.Poisson.loss(m, [ur, rho], blank, f)
        pu, = torch.autograd.grad(pen, ur)
        pen = pen.detach()
        out = dict(kwargs=repr(kw), u=T(u), rho=T(rho), inputs=T(inputs), f=T(f), loss=np.float32(T(loss)), loss_du=T(lu), loss_drho=T(lr),
                   compliance=np.float32(T(comp)), compliance_du=T(cu), compliance_drho=T(cr), dbc=np.float32(T(pen)), dbc_du=T(pu))
        np.savez_compressed(os.path.join(outdir, f"loss_topopt_n{n}.npz"), **out)
        print("topopt", n, float(loss), float(comp), float(pen), float(lr.abs().max()))
    with open(os.path.join(outdir, "PROVENANCE_topopt.txt"), "w") as fh:
        fh.write("loss_topopt_n17.npz, loss_topopt_n33.npz: written by tools/gen_golden_topopt.py from the reference's\n"
                 "examples/poisson/single_instance/16_topopt.py (Poisson.loss, Poisson.compliance called unbound on seeded inputs; float32,\n"
                 "CPU, autograd gradients).  Data only: inputs and recorded outputs.  Regenerate with the reference repository present:\n"
                 "    python tools/gen_golden_topopt.py\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    a = ap.parse_args()
    install_shims()
    torch.manual_seed(0)
    gen(a.out)


if __name__ == "__main__":
    main()
