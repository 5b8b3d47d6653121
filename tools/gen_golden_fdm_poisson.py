#!/usr/bin/env python3
"""Golden vectors of the finite-difference Poisson residual losses from the *imported* reference scripts.

Like tools/gen_golden_eikonal3d.py (whose shims it reuses), this runs only where the reference repository is present.  It imports the
three DiffNetFDM scripts under examples/poisson/single_instance/ as modules and calls their own loss bodies, Poisson.loss, unbound, on a
reference DiffNetFDM instance built by the library constructor.  Only data -- inputs and the reference's outputs -- is written, to
tests/golden/loss_fdm_poisson_*.npz, batch 1.

  loss_fdm_poisson_mms_n9.npz         12_fdm_mms.py        9^2 nodes: ||f + grad u . grad nu + nu lap u||_2 per sample, one condition (u = 0)
  loss_fdm_poisson_klsum_n12.npz      12_klsum_fdm.py      12^2 nodes: (grad u . grad nu + nu lap u)^2 per node, two conditions (1 | 0)
  loss_fdm_poisson_klsum_nbc_n9.npz   12_klsum_fdm_nbc.py  9^2 nodes: the same plus 0.1 x the mean of the two Neumann row terms

The inputs have the layout of the scripts' datasets (inputs_tensor = nu, bc1, bc2; forcing_tensor = f) with seeded fields in place of
the datasets' files: nu = exp of a smooth field plus noise (so that grad nu matters), u = a smooth field plus noise of the same size,
f = seeded noise scaled like lap u.  The conditions sit where the datasets put them: klsum: bc1 the column x = 0 (u = 1), bc2 the
column x = 1 (u = 0); mms: bc2 the whole boundary (the script applies bc2 only).

Each file holds: script, n, u, inputs (1,3,n,n), forcing (1,1,n,n), the reference's sobelx / sobely / sobelxx / sobelyy parameters, the
loss tensor the body returns (`loss`), its mean (`loss_mean`: what the script's training step minimises) and `grad`, the autograd
gradient of that mean with respect to u.

Usage: python tools/gen_golden_fdm_poisson.py [--out tests/golden]
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import T, install_shims, load_script, make, rng  # noqa: E402

DIR = "examples/poisson/single_instance/"
CASES = (("mms_n9", "12_fdm_mms.py", 9, 201), ("klsum_n12", "12_klsum_fdm.py", 12, 203), ("klsum_nbc_n9", "12_klsum_fdm_nbc.py", 9, 205))

PROVENANCE = """loss_fdm_poisson_*.npz: written by tools/gen_golden_fdm_poisson.py from the reference's own loss bodies, called unbound on a
reference DiffNetFDM instance:
  loss_fdm_poisson_mms_n9.npz         examples/poisson/single_instance/12_fdm_mms.py::Poisson.loss, 9^2 nodes
  loss_fdm_poisson_klsum_n12.npz      examples/poisson/single_instance/12_klsum_fdm.py::Poisson.loss, 12^2 nodes
  loss_fdm_poisson_klsum_nbc_n9.npz   examples/poisson/single_instance/12_klsum_fdm_nbc.py::Poisson.loss, 9^2 nodes
Data only: the seeded inputs (u, inputs = nu | bc1 | bc2, forcing), the reference's sobel* parameters, the loss tensor the body
returns, its mean and the autograd gradient of the mean with respect to u.  Batch 1.
"""


def fields(n, seed, mms):
    g = rng(seed)
    x = torch.linspace(0.0, 1.0, n)
    xx, yy = x[None, :].expand(n, n), x[:, None].expand(n, n)
    nu = torch.exp(0.6 * torch.sin(2.0 * xx + 1.0) * torch.cos(3.0 * yy) + 0.2 * (2.0 * torch.rand((n, n), generator=g) - 1.0))
    u = torch.sin(np.pi * xx) * torch.sin(np.pi * yy) + 1.0 - xx + 0.3 * (2.0 * torch.rand((n, n), generator=g) - 1.0)
    f = (n - 1) ** 2 * 0.3 * (2.0 * torch.rand((n, n), generator=g) - 1.0)
    bc1, bc2 = torch.zeros(n, n), torch.zeros(n, n)
    if mms:
        bc2[0, :] = bc2[-1, :] = bc2[:, 0] = bc2[:, -1] = 1.0
    else:
        bc1[:, 0] = 1.0
        bc2[:, -1] = 1.0
    inputs = torch.stack((nu, bc1, bc2)).reshape(1, 3, n, n).float()
    return u.reshape(1, 1, n, n).float(), inputs, f.reshape(1, 1, n, n).float()


def gen(outdir):
    from DiffNet.DiffNetFDM import DiffNetFDM
    for tag, script, n, seed in CASES:
        mod = load_script(DIR + script, "ref_fdm_" + tag)
        m = make(mod.Poisson, DiffNetFDM, domain_size=n)
        u, inputs, forcing = fields(n, seed, tag.startswith("mms"))
        ur = u.clone().requires_grad_(True)
        with contextlib.redirect_stdout(io.StringIO()):
            loss = mod.Poisson.loss(m, ur, inputs, forcing)
        mean = loss.mean()
        grad, = torch.autograd.grad(mean, ur)
        out = dict(script=DIR + script + "::Poisson.loss", n=np.int64(n), u=T(u), inputs=T(inputs), forcing=T(forcing),
                   sobelx=T(m.sobelx), sobely=T(m.sobely), sobelxx=T(m.sobelxx), sobelyy=T(m.sobelyy),
                   loss=T(loss), loss_mean=np.float32(T(mean)), grad=T(grad))
        np.savez_compressed(os.path.join(outdir, f"loss_fdm_poisson_{tag}.npz"), **out)
        print("fdm_poisson", tag, "loss", tuple(loss.shape), "mean", float(mean), "max|grad|", float(grad.abs().max()))
    with open(os.path.join(outdir, "PROVENANCE_fdm_poisson.txt"), "w") as fh:
        fh.write(PROVENANCE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    a = ap.parse_args()
    install_shims()
    torch.manual_seed(0)
    gen(a.out)


if __name__ == "__main__":
    main()
