#!/usr/bin/env python3
"""Topology optimisation of a heat sink on nodal parameters: the alternating loop of the reference's
examples/poisson/single_instance/16_topopt.py on MI355X kernels, without Lightning.

Two nodal fields are optimised, the temperature u and the raw design field rho with nu = 0.001 + sigmoid(rho)^3.  Every epoch takes one
Adam step on each of three objectives, each with its own optimiser, as in the reference:

    energy      mean sum_g W (0.5 nu |grad u|^2 - u f), u = 0 on the sink (the left and bottom edges)   -> u and rho
    compliance  mean sum_g W (-u f)                                                                     -> u
    volume      (sum nu - 0.4 N^2)^2                                                                    -> rho

    python examples/topopt_2d.py [--size 64] [--epochs 20] [--mode fused|composed]

--mode fused differentiates the energy with respect to nu with dn_poisson_coef_grad (one launch in the backward pass); --mode composed sets
dn_config_set("COEF_GRAD", "composed"): the same loss differentiated through the Gauss-point operators, as before that launch existed.
Prints the three values per epoch; --dump FILE saves the final fields."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd import DiffNet2DFEM, _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    _lib.config_set("COEF_GRAD", "composed" if a.mode == "composed" else "")
    dev = torch.device("cuda:0")
    n = a.size
    m = DiffNet2DFEM(None, domain_size=n).to(dev)
    g = torch.Generator().manual_seed(42)
    u = torch.nn.Parameter((0.1 * torch.rand((1, 1, n, n), generator=g)).to(dev))
    rho = torch.nn.Parameter((0.2 * torch.rand((1, 1, n, n), generator=g) - 0.1).to(dev))
    f = torch.ones((1, 1, n, n), device=dev)
    sink = torch.zeros((1, 1, n, n), device=dev)
    sink[..., :, 0] = 1
    sink[..., 0, :] = 1
    dirichlet = [(sink, 0.0)]
    target = 0.4 * n * n
    opts = [torch.optim.Adam([u, rho], lr=a.lr), torch.optim.Adam([u], lr=a.lr), torch.optim.Adam([rho], lr=a.lr)]

    def nu_of(r):
        return 0.001 + torch.sigmoid(r) ** 3

    objectives = [lambda: m.energy_loss(u, nu_of(rho), f, dirichlet=dirichlet, c=0.5),
                  lambda: m.energy_loss(u, None, f, dirichlet=dirichlet, c=0.0),
                  lambda: (nu_of(rho).sum() - target) ** 2]
    for epoch in range(a.epochs):
        vals = []
        for opt, fn in zip(opts, objectives):
            opt.zero_grad(set_to_none=True)
            val = fn()
            val.backward()
            opt.step()
            vals.append(val.detach())
        e, c, v = (float(x) for x in vals)
        print(f"epoch {epoch:4d}  energy {e:+.8e}  compliance {c:+.8e}  volume {v:.8e}", flush=True)
    if a.dump:
        torch.save({"u": u.detach().cpu(), "rho": rho.detach().cpu(), "values": [float(x) for x in vals]}, a.dump)


if __name__ == "__main__":
    main()
