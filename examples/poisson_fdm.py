#!/usr/bin/env python3
"""Finite-difference Poisson problems on the unit square, solved for the nodal field itself -- the three DiffNetFDM scripts of the
reference under examples/poisson/single_instance/ without Lightning or plotting:

    --case mms        12_fdm_mms.py         -div(grad u) = f, u = sin(pi x) sin(pi y): || f + grad u . grad nu + nu lap u ||_2, u = 0 on the boundary
           klsum      12_klsum_fdm.py       -div(nu grad u) = 0, nu = exp(KL sum): mean (grad u . grad nu + nu lap u)^2, u = 1 | 0 at x = 0 | 1
           klsum_nbc  12_klsum_fdm_nbc.py   the same plus 0.1 x the mean of the two Neumann row terms (u[0] - u[1])^2 + (u[-1] - u[-2])^2

with the derivatives taken by the class's 3x3 `sobel*` kernels as valid convolutions.  The scripts' loss body (two torch.where, six conv2d
calls, six elementwise passes, the sum of squares or norm and the autograd backward through all of it) is ONE launch for the two
mean-of-squares losses and two for the norm (DiffNetFDM.poisson_residual_loss, dn_fdm_poisson_apply).  The datasets are the ported
ones (RectangleManufactured, klsum.Dataset); without --coeff the KL coefficients are six seeded normal draws.

    python examples/poisson_fdm.py [--case mms|klsum|klsum_nbc] [--n 64] [--mode fused|composed] [--optimizer lbfgs|adam] [--steps 20]

--mode fused     the fused HIP operator
       composed  the same loss from torch's own operators, as the scripts compose it (DiffNetFDM.composed_poisson_residual_loss)
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd.datasets.single_instances.klsum import Dataset  # noqa: E402
from diffnet_amd.datasets.single_instances.rectangles import RectangleManufactured  # noqa: E402
from diffnet_amd.fdm import DiffNetFDM  # noqa: E402

CASES = ("mms", "klsum", "klsum_nbc")


class Poisson(DiffNetFDM):
    """One nodal parameter, one sample of the case's dataset."""

    def __init__(self, field, dataset, n, case, mode):
        super().__init__(None, None, domain_size=n)
        self.net, self.case, self.mode = field, case, mode
        inputs, forcing = dataset[0]
        for name, t in (("nu", inputs[0:1]), ("bc1", inputs[1:2]), ("bc2", inputs[2:3]), ("f", forcing)):
            self.register_buffer(name, t.reshape(1, 1, n, n).contiguous())
        x = np.linspace(0.0, 1.0, n)
        xx, yy = np.meshgrid(x, x)
        self.register_buffer("u_exact", torch.from_numpy((np.sin(np.pi * xx) * np.sin(np.pi * yy)).astype(np.float32))[None, None].contiguous())

    def loss(self):
        fn = self.poisson_residual_loss if self.mode == "fused" else self.composed_poisson_residual_loss
        u = self.net[0]
        if self.case == "mms":               # the script applies bc2 only
            return fn(u, self.nu, self.f, bc=(None, self.bc2), bc_values=(0.0, 0.0), norm="l2", fs=1.0)
        return fn(u, self.nu, None, bc=(self.bc1, self.bc2), bc_values=(1.0, 0.0), norm="mean_sq", neumann=0.1 if self.case == "klsum_nbc" else 0.0)

    def solution(self):
        u = self.net[0].detach()
        if self.case != "mms":
            u = torch.where(self.bc1 > 0.5, torch.ones_like(u), u)
        return torch.where(self.bc2 > 0.5, torch.zeros_like(u), u)


def run(case="mms", n=64, steps=20, optimizer="lbfgs", mode="fused", lr=3e-4, coeff=None, verbose=True):
    if case not in CASES:
        raise ValueError(f"case must be one of {CASES}, got {case!r}")
    if mode not in ("fused", "composed"):
        raise ValueError(f"mode must be 'fused' or 'composed', got {mode!r}")
    dev = torch.device("cuda")
    if case == "mms":
        dataset = RectangleManufactured(domain_size=n)
    elif coeff is not None:
        dataset = Dataset(coeff, domain_size=n)
    else:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "coefficients.txt")
            np.savetxt(path, np.random.default_rng(42).standard_normal(6))
            dataset = Dataset(path, domain_size=n)
    field = nn.ParameterList([nn.Parameter(torch.ones(1, 1, n, n, device=dev))])      # the scripts start from u = 1
    m = Poisson(field, dataset, n, case, mode).to(dev)
    if optimizer == "lbfgs":
        # the scripts' settings: 12_fdm_mms.py:142 | 12_klsum_fdm.py, 12_klsum_fdm_nbc.py:180
        opt = torch.optim.LBFGS(field, lr=0.1, max_iter=4) if case == "mms" else torch.optim.LBFGS(field, lr=1.0, max_iter=5)
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
            print(f"step {it:4d}  loss {hist[-1]:.6e}")
    with torch.no_grad():
        hist.append(float(m.loss()))
    torch.cuda.synchronize()
    if verbose:
        u = m.solution()
        tail = f"; || u - u_exact || / n = {float(torch.linalg.vector_norm(u - m.u_exact)) / n:.4e}" if case == "mms" else \
            f"; u in [{float(u.min()):.3f}, {float(u.max()):.3f}]"
        print(f"{steps} steps in {time.perf_counter() - t0:.2f} s ({case}, {mode}, {optimizer}, {n}^2 nodes); loss {hist[0]:.6e} -> {hist[-1]:.6e}" + tail)
    return field[0].detach(), hist


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=CASES, default="mms")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    ap.add_argument("--optimizer", choices=("lbfgs", "adam"), default="lbfgs")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--coeff", default=None, help="KL coefficient file of the klsum cases (np.loadtxt)")
    a = ap.parse_args()
    run(a.case, a.n, a.steps, a.optimizer, a.mode, a.lr, a.coeff)


if __name__ == "__main__":
    main()
