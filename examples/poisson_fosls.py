#!/usr/bin/env python3
"""Manufactured Poisson problem on the unit square as a first-order system: minimise the least-squares loss over the nodal fields u and
the flux (mx, my), held in one packed (1, 3, n, n) parameter -- the set-up of
`examples/poisson/single_instance/11_manufactured_strong_form_two_dofs.py` of the reference (its dataset RectangleManufactured: nu = 1,
u = 0 on the wall through condition 2, forcing 2 pi^2 sin(pi x) sin(pi y); exact solution sin(pi x) sin(pi y)), without Lightning:

    loss = mean over elements of sum_g w_g ( |m - nu grad u|^2 + (div m + f)^2 )

The script's loss body (11 Gauss-point evaluations, elementwise passes over (B, G, nel, nel) tensors and the autograd backward through all
of it) is ONE launch (diffnet_amd.fosls.fosls_loss) that reads the packed parameter in place and writes the loss and the packed gradient.

    python examples/poisson_fosls.py [--n 512] [--degree 1] [--steps 30] [--optimizer lbfgs|adam] [--mode fused|composed]

--mode fused     fosls_loss: the fused HIP operator
       composed  fosls_loss_composed: the same loss on the drop-in operators (gauss_pt_evaluation*)
Prints the error of u against sin(pi x) sin(pi y) as the script does (the 2-norm of the nodal difference over n).
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from DiffNet.DiffNetFEM import DiffNet2DFEM  # noqa: E402  (reference import path, MI355X implementation)
from diffnet_amd.fosls import fosls_loss, fosls_loss_composed  # noqa: E402


class PoissonFosls(DiffNet2DFEM):
    """The script's module: one packed nodal parameter (u, mx, my), the dataset's coefficient, masks and forcing."""

    def __init__(self, fields, n, degree=1, mode="fused"):
        super().__init__(None, None, domain_size=n, fem_basis_deg=degree)
        self.net, self.mode = fields, mode
        x = np.linspace(0.0, 1.0, n)
        xx, yy = np.meshgrid(x, x)
        exact = np.sin(math.pi * xx) * np.sin(math.pi * yy)
        bc2 = np.zeros((n, n), dtype=bool)
        bc2[0, :] = bc2[-1, :] = bc2[:, 0] = bc2[:, -1] = True
        self.register_buffer("nu", torch.ones((1, 1, n, n)))
        self.register_buffer("bc1", torch.zeros((1, 1, n, n), dtype=torch.bool))
        self.register_buffer("bc2", torch.from_numpy(bc2)[None, None].contiguous())
        self.register_buffer("forcing", torch.from_numpy((2.0 * math.pi ** 2 * exact).astype(np.float32))[None, None].contiguous())
        self.register_buffer("u_exact", torch.from_numpy(exact.astype(np.float32))[None, None].contiguous())

    def loss(self):
        fn = fosls_loss if self.mode == "fused" else fosls_loss_composed
        return fn(self, self.net[0], nu=self.nu, bc=(self.bc1, self.bc2), bc_values=(1.0, 0.0), f=self.forcing)

    def error(self):
        """The script's figure: || u~ - u_exact ||_2 / n over the nodes, u~ after the conditions"""
        u = self.net[0].detach()[:, 0:1]
        u = torch.where(self.bc2, torch.zeros_like(u), torch.where(self.bc1, torch.ones_like(u), u))
        return float(torch.linalg.vector_norm(u - self.u_exact)) / u.shape[-1]


def run(n=512, degree=1, steps=30, optimizer="lbfgs", mode="fused", lr=1e-2, verbose=True, seed=0):
    if (n - 1) % degree:
        raise ValueError(f"degree-{degree} elements need (n - 1) % {degree} == 0 nodes per axis")
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(seed)
    fields = nn.ParameterList([nn.Parameter(torch.randn((1, 3, n, n), generator=g).to(dev))])       # the script starts from randn
    m = PoissonFosls(fields, n, degree, mode).to(dev)
    if optimizer == "lbfgs":
        opt = torch.optim.LBFGS(fields, lr=1.0, max_iter=5)                                 # the script's configure_optimizers
    elif optimizer == "adam":
        opt = torch.optim.Adam(fields, lr=lr)
    else:
        raise ValueError(f"optimizer must be 'lbfgs' or 'adam', got {optimizer!r}")
    hist = []

    def closure():
        opt.zero_grad(set_to_none=True)
        loss = m.loss()
        loss.backward()
        return loss

    t0 = time.perf_counter()
    for it in range(steps):
        loss = opt.step(closure)
        hist.append(float(loss))
        if verbose:
            print(f"step {it:4d}  loss {hist[-1]:.6e}  error of u {m.error():.4e}")
    torch.cuda.synchronize()
    if verbose:
        print(f"{steps} steps in {time.perf_counter() - t0:.2f} s ({mode}, {optimizer}, {n}^2 nodes Q{degree}); "
              f"|| u - sin(pi x) sin(pi y) || / n = {m.error():.4e}")
    return fields[0].detach(), hist


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    ap.add_argument("--optimizer", choices=("lbfgs", "adam"), default="lbfgs")
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--degree", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--lr", type=float, default=1e-2)
    a = ap.parse_args()
    run(a.n, a.degree, a.steps, a.optimizer, a.mode, a.lr)


if __name__ == "__main__":
    main()
