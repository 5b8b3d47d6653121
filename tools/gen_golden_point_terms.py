#!/usr/bin/env python3
"""Golden vectors of the point-cloud term from the *imported* reference scripts.

Like tools/gen_golden_fdm_poisson.py, this runs only where the reference repository is present.  It imports the two point-cloud Poisson
scripts under examples/poisson/single_instance/ as modules and calls their own loss bodies, Poisson.loss, unbound, on a reference
DiffNet2DFEM instance built by the library constructor and converted to float64.  The bodies call `self.bf_1d_th` and
`self.bf_1d_der_th`, which the reference library does not define: the generator sets them on the object, as the linear 1-D basis
(1 -+ x) / 2 and its derivative (as tools/gen_golden_eikonal3d.py does).

  point_terms_disk_n9.npz       pc_poisson_disk.py                    9^2 nodes
  point_terms_immersed_n9.npz   pc_complex_immersed_background.py     9^2 nodes

The loss of both bodies is  mean(energy) + sum_p (u(x_p) - 1)^2  with u(x_p) the bilinear interpolant at the point, x indexing ROWS
(`u[b, 0, nidx, nidy]`).  Each body is called twice on the same u: with a cloud A of 40 points and with a cloud A1 of one point.  The
energy term is the same in both calls, so loss(A) - loss(A1) and grad(A) - grad(A1) are differences of the point term alone.  Cloud A
holds a point exactly on an interior element boundary (x = 3 h) and one at x = 0; none at x = L, where the body indexes out of range.

Each file holds data only: script, n, u (1,1,9,9), cloud_a (40,2), cloud_a1 (1,2), loss_a, loss_a1, grad_a, grad_a1, all float64.

Usage: python tools/gen_golden_point_terms.py [--out tests/golden]
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
CASES = (("disk_n9", "pc_poisson_disk.py", 9, 301), ("immersed_n9", "pc_complex_immersed_background.py", 9, 303))

PROVENANCE = """point_terms_*.npz: written by tools/gen_golden_point_terms.py from the reference's own loss bodies, called unbound on a reference
DiffNet2DFEM instance in float64:
  point_terms_disk_n9.npz       examples/poisson/single_instance/pc_poisson_disk.py::Poisson.loss, 9^2 nodes
  point_terms_immersed_n9.npz   examples/poisson/single_instance/pc_complex_immersed_background.py::Poisson.loss, 9^2 nodes
Data only: the seeded field u, a cloud of 40 points (one exactly on an interior element boundary, one at x = 0, none at x = L) and a
cloud of one point, and for each cloud the loss the body returns and its autograd gradient with respect to u.  The energy term of the
bodies cancels in loss_a - loss_a1 and grad_a - grad_a1: what is left is the point term sum_p (u(x_p) - 1)^2 with x indexing rows.
bf_1d_th / bf_1d_der_th, which the bodies call and the reference library does not define, were set by the generator to the linear 1-D
basis (1 -+ x) / 2 and its derivative.
"""


def clouds(n, seed):
    g = rng(seed)
    h = 1.0 / (n - 1)
    a = 0.02 + 0.96 * torch.rand((40, 2), generator=g, dtype=torch.float64)
    a[0] = torch.tensor([3 * h, 0.3])            # exactly on an interior element boundary
    a[1] = torch.tensor([0.0, 0.6])              # on the face x = 0
    a1 = torch.tensor([[0.52, 0.31]], dtype=torch.float64)
    x = torch.linspace(0.0, 1.0, n, dtype=torch.float64)
    u = torch.sin(2.0 * x[:, None] + 0.3) * torch.cos(1.5 * x[None, :]) + 0.8 + 0.2 * (2.0 * torch.rand((n, n), generator=g, dtype=torch.float64) - 1.0)
    return u.reshape(1, 1, n, n), a, a1


def gen(outdir):
    from DiffNet.DiffNetFEM import DiffNet2DFEM
    for tag, script, n, seed in CASES:
        mod = load_script(DIR + script, "ref_pc_" + tag)
        m = make(mod.Poisson, DiffNet2DFEM, domain_size=n).double()
        m.bf_1d_th = lambda x: torch.stack((0.5 * (1.0 - x), 0.5 * (1.0 + x)))
        m.bf_1d_der_th = lambda x: torch.stack((-0.5 * torch.ones_like(x), 0.5 * torch.ones_like(x)))
        u, a, a1 = clouds(n, seed)
        out = dict(script=DIR + script + "::Poisson.loss", n=np.int64(n), u=T(u), cloud_a=T(a), cloud_a1=T(a1))
        for name, pc in (("a", a), ("a1", a1)):
            inputs = torch.stack((pc, torch.zeros_like(pc)))[None]           # (1, 2, P, 2): points | normals (unused by the body)
            ur = u.clone().requires_grad_(True)
            with contextlib.redirect_stdout(io.StringIO()):
                loss = mod.Poisson.loss(m, ur, inputs, torch.ones_like(u))
            grad, = torch.autograd.grad(loss, ur)
            out["loss_" + name], out["grad_" + name] = np.float64(T(loss)), T(grad)
        np.savez_compressed(os.path.join(outdir, f"point_terms_{tag}.npz"), **out)
        print("point_terms", tag, "loss(A) - loss(A1)", float(out["loss_a"] - out["loss_a1"]), "max|dgrad|", float(np.abs(out["grad_a"] - out["grad_a1"]).max()))
    with open(os.path.join(outdir, "PROVENANCE_point_terms.txt"), "w") as fh:
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
