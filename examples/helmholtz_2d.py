#!/usr/bin/env python3
"""The two Helmholtz problems of the reference on the unit square, -div(nu grad u) - k^2 u = f with u = 0 on the wall, solved for the nodal
field itself -- the set-up of `examples/poisson/single_instance/14_helmholtz_mms.py` (dataset RectangleHelmholtzManufactured: k = 0.5,
f = (2 pi^2 - k^2) sin(pi x) sin(pi y), exact solution sin(pi x) sin(pi y)) and `14_helmholtz_ddelta.py` (RectangleHelmholtzDeltaForce:
k = 1 / 8, a Gaussian point source), without Lightning:

    energy   = mean over elements of sum_g w_g ( 0.5 (nu |grad u|^2 - k^2 u^2) - u f )          the scripts' loss
    residual = sum over nodes of R^2, R the assembled weak-form residual                           well posed also for k^2 > 2 pi^2

The scripts' loss body (5 Gauss-point evaluations, elementwise passes over (B, G, nel, nel) tensors and the autograd backward through all
of it) is ONE launch (diffnet_amd.helmholtz.helmholtz_energy_loss); the residual loss is two.

    python examples/helmholtz_2d.py [--case mms|ddelta] [--n 64] [--degree 1] [--mode fused|composed] [--loss energy|residual]
                                    [--optimizer lbfgs|adam] [--steps 5]

--mode fused     the fused HIP operator (dn_helmholtz_apply)
       composed  the same losses on the drop-in operators (gauss_pt_evaluation* and their adjoints)
For `mms` it prints the error against sin(pi x) sin(pi y) as the script does (the 2-norm of the nodal difference over n).
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
from diffnet_amd import helmholtz as hh  # noqa: E402
from diffnet_amd.datasets.single_instances.rectangles import RectangleHelmholtzDeltaForce, RectangleHelmholtzManufactured  # noqa: E402

DATASETS = dict(mms=RectangleHelmholtzManufactured, ddelta=RectangleHelmholtzDeltaForce)


class Helmholtz(DiffNet2DFEM):
    """The scripts' module: one nodal parameter, the dataset's coefficient, masks, forcing and khh."""

    def __init__(self, field, case, n, degree=1, mode="fused", loss="energy"):
        super().__init__(None, None, domain_size=n, fem_basis_deg=degree)
        dataset = DATASETS[case](domain_size=n)
        inputs, forcing = dataset[0]
        self.net, self.case, self.mode, self.loss_kind, self.khh = field, case, mode, loss, dataset.khh
        self.register_buffer("nu", inputs[None, 0:1].contiguous())
        self.register_buffer("bc1", inputs[None, 1:2].contiguous())
        self.register_buffer("bc2", inputs[None, 2:3].contiguous())
        self.register_buffer("forcing", forcing[None].contiguous())
        x = np.linspace(0.0, 1.0, n)
        xx, yy = np.meshgrid(x, x)
        self.register_buffer("u_exact", torch.from_numpy((np.sin(math.pi * xx) * np.sin(math.pi * yy)).astype(np.float32))[None, None].contiguous())

    def inputs(self):
        return dict(nu=self.nu, bc=(self.bc1, self.bc2), bc_values=(1.0, 0.0), f=self.forcing)

    def loss(self):
        coef = hh.helmholtz_coefficients(self.khh)
        if self.loss_kind == "energy":
            fn = hh.helmholtz_energy_loss if self.mode == "fused" else hh.helmholtz_energy_loss_composed
            return fn(self, self.net[0], **self.inputs(), **coef)
        if self.mode == "fused":
            return hh.helmholtz_residual_loss(self, self.net[0], sigma=coef["sigma"], **self.inputs())
        return torch.sum(hh.helmholtz_residual_composed(self, self.net[0], sigma=coef["sigma"], **self.inputs()) ** 2)

    def error(self):
        """The script's figure: || u~ - u_exact ||_2 / n over the nodes, u~ after the conditions"""
        u = self.net[0].detach()
        u = torch.where(self.bc2 > 0.5, torch.zeros_like(u), torch.where(self.bc1 > 0.5, torch.ones_like(u), u))
        return float(torch.linalg.vector_norm(u - self.u_exact)) / u.shape[-1]


def run(case="mms", n=64, degree=1, steps=5, optimizer="lbfgs", mode="fused", loss="energy", lr=1e-2, verbose=True):
    if case not in DATASETS:
        raise ValueError(f"case must be 'mms' or 'ddelta', got {case!r}")
    if loss not in ("energy", "residual"):
        raise ValueError(f"loss must be 'energy' or 'residual', got {loss!r}")
    if (n - 1) % degree:
        raise ValueError(f"degree-{degree} elements need (n - 1) % {degree} == 0 nodes per axis")
    dev = torch.device("cuda")
    field = nn.ParameterList([nn.Parameter(torch.ones((1, 1, n, n), device=dev))])               # the scripts start from ones
    m = Helmholtz(field, case, n, degree, mode, loss).to(dev)
    if optimizer == "lbfgs":
        opt = torch.optim.LBFGS(field, lr=1.0, max_iter=5)                                  # the scripts' configure_optimizers
    elif optimizer == "adam":
        opt = torch.optim.Adam(field, lr=lr)
    else:
        raise ValueError(f"optimizer must be 'lbfgs' or 'adam', got {optimizer!r}")
    hist = []

    def closure():
        opt.zero_grad(set_to_none=True)
        val = m.loss()
        val.backward()
        return val

    t0 = time.perf_counter()
    for it in range(steps):
        val = opt.step(closure)
        hist.append(float(val))
        if verbose:
            print(f"step {it:4d}  loss {hist[-1]:.6e}" + (f"  error of u {m.error():.4e}" if case == "mms" else ""))
    with torch.no_grad():
        hist.append(float(m.loss()))
    torch.cuda.synchronize()
    if verbose:
        print(f"{steps} steps in {time.perf_counter() - t0:.2f} s ({case}, {loss}, {mode}, {optimizer}, {n}^2 nodes Q{degree}); final loss {hist[-1]:.6e}"
              + (f"; || u - u_exact || / n = {m.error():.4e}" if case == "mms" else ""))
    return field[0].detach(), hist


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=("mms", "ddelta"), default="mms")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--degree", type=int, default=1)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    ap.add_argument("--loss", choices=("energy", "residual"), default="energy")
    ap.add_argument("--optimizer", choices=("lbfgs", "adam"), default="lbfgs")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--lr", type=float, default=1e-2)
    a = ap.parse_args()
    run(a.case, a.n, a.degree, a.steps, a.optimizer, a.mode, a.loss, a.lr)


if __name__ == "__main__":
    main()
