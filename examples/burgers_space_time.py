#!/usr/bin/env python3
"""Space-time Burgers on [-1, 1] x [0, 1] (y is time) by minimising the strong-form least-squares loss over the nodal field u -- the
set-up of `examples/burgers/single_instance/01_2d_space_time.py` of the reference (Q2 elements; its dataset's condition 1 puts cos(4 pi x)
on the first node column, condition 2 zero on the first and last node row), without Lightning:

    loss = mean over elements of sum_g w_g (u_t + u u_x - nu u_xx)^2

The script's loss body (4 Gauss-point evaluations on Q2 tables, elementwise passes over (B, 9, nely, nelx) tensors and the autograd
backward through all of it) is ONE launch (diffnet_amd.strongform.strong_form_loss) that writes the loss and its gradient.

    python examples/burgers_space_time.py [--n 257] [--steps 30] [--optimizer lbfgs|adam] [--viscosity 0] [--mode fused|composed]

--mode fused     strong_form_loss: the fused HIP operator
       composed  strong_form_loss_composed: the same loss on the drop-in operators (gauss_pt_evaluation*, _der2_x included)
--viscosity      nu of the viscous form (the script's dataset carries 0.01 / pi but its loss leaves u_xx out: 0)
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
from diffnet_amd.strongform import burgers_coefficients, strong_form_loss, strong_form_loss_composed  # noqa: E402


def burgers_dataset(n):
    """The masks and values of the script's Burg2DXT: condition 1 on the first node column takes cos(4 pi x) of the x grid, condition 2
    on the first and last node row sets 0 (applied second: it wins in the corners)."""
    x = np.linspace(-1.0, 1.0, n)
    bc1 = np.zeros((n, n), dtype=bool)
    bc1[:, 0] = True
    v1 = np.zeros((n, n), dtype=np.float32)
    v1[:, 0] = np.cos(2 * math.pi * 2 * x)
    bc2 = np.zeros((n, n), dtype=bool)
    bc2[0, :] = True
    bc2[-1, :] = True
    return bc1, v1, bc2


class BurgersXT(DiffNet2DFEM):
    """The script's module in its `no_network` mode: one nodal parameter field, the dataset's two masks."""

    def __init__(self, field, n, viscosity=0.0, mode="fused"):
        super().__init__(None, None, domain_size=n, fem_basis_deg=2)
        self.net_u, self.mode = field, mode
        bc1, v1, bc2 = burgers_dataset(n)
        self.register_buffer("bc1", torch.from_numpy(bc1)[None, None].contiguous())
        self.register_buffer("bc2", torch.from_numpy(bc2)[None, None].contiguous())
        self.register_buffer("v1", torch.from_numpy(v1)[None, None].contiguous())
        self.coef = burgers_coefficients(viscosity)

    def loss(self):
        fn = strong_form_loss if self.mode == "fused" else strong_form_loss_composed
        return fn(self, self.net_u[0], (self.bc1, self.bc2), (self.v1, 0.0), coef=self.coef)


def run(n=257, steps=30, optimizer="lbfgs", viscosity=0.0, mode="fused", lr=1e-2, verbose=True, seed=0):
    if (n - 1) % 2:
        raise ValueError("Q2 elements need an odd number of nodes per axis")
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    field = nn.ParameterList([nn.Parameter(torch.ones((1, 1, n, n), device=dev))])         # the script starts from u = 1
    m = BurgersXT(field, n, viscosity, mode).to(dev)
    if optimizer == "lbfgs":
        opt = torch.optim.LBFGS(field, lr=1.0, max_iter=5)                                  # the script's configure_optimizers
    elif optimizer == "adam":
        opt = torch.optim.Adam(field, lr=lr)
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
            print(f"step {it:4d}  loss {hist[-1]:.6e}")
    torch.cuda.synchronize()
    if verbose:
        print(f"{steps} steps in {time.perf_counter() - t0:.2f} s ({mode}, {optimizer}, {n}^2 nodes Q2, nu = {viscosity:g})")
    return field[0].detach(), hist


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    ap.add_argument("--viscosity", type=float, default=0.0)
    ap.add_argument("--optimizer", choices=("lbfgs", "adam"), default="lbfgs")
    ap.add_argument("--n", type=int, default=257)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--lr", type=float, default=1e-2)
    a = ap.parse_args()
    run(a.n, a.steps, a.optimizer, a.viscosity, a.mode, a.lr)


if __name__ == "__main__":
    main()
