#!/usr/bin/env python3
"""Navier-Stokes flow in the lid-driven cavity, solved by minimising the norms of the three VMS-stabilised weak-form residuals over the
nodal fields (u, v, p) -- the flow of the reference's `examples/navier-stokes/single_instance/e1_ns_ldc_resmin.py` in its `no_network`
mode (three nodal parameter fields, no-slip walls on u and v, the lid profile u = 1 - 16 (x - 0.5)^4, the pressure pinned at one corner,
one Adam optimiser per field stepping on its own residual norm) without Lightning.  The script's residual body (:176-308: 13 Gauss-point
evaluations, ~60 elementwise passes, three masks on the inputs, three assemblies, three masks on the residuals) is ONE launch
(diffnet_amd.navier_stokes.ns_loss), its backward for all three norms another.

`--stokes-steps N` first runs N steps on the Stokes (PSPG) residual norms (diffnet_amd.stokes.stokes_loss, the coefficients of the
Navier-Stokes scripts' Stokes stage), mirroring the Stokes -> Navier-Stokes staging of the e2 scripts.

Coefficients as in the script: visco = 1/Re, wscale = (h/2)^2, tau_h = (h, h), cinv = 36.

    python examples/ns_ldc.py [--size 64] [--steps 200] [--lr 5e-4] [--re 100] [--stokes-steps 0] [--mode fused|composed]

--mode fused     ns_loss: the fused HIP operator
       composed  ns_residuals_composed + torch.norm: the same residuals on the drop-in operators (gauss_pt_evaluation*, assemble)
"""
import argparse
import os
import sys
import time

import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from DiffNet.DiffNetFEM import DiffNet2DFEM  # noqa: E402  (reference import path, MI355X implementation)
from diffnet_amd.navier_stokes import ns_loss, ns_residuals_composed  # noqa: E402
from diffnet_amd.stokes import stokes_loss, stokes_residuals_composed  # noqa: E402


class NSLDC(DiffNet2DFEM):
    """The reference's `NS_LDC` (e1_ns_ldc_resmin.py:95-132): three field "networks", the cavity's masks and lid."""

    def __init__(self, fields, Re=100.0, mode="fused", **kwargs):
        super().__init__(None, **kwargs)
        self.net_u, self.net_v, self.net_p = fields
        self.mode = mode
        n = self.domain_size
        self.Re = Re
        self.viscosity = 1.0 / Re
        walls = torch.zeros((1, 1, n, n))
        walls[..., 0, :] = 1.0
        walls[..., -1, :] = 1.0
        walls[..., :, 0] = 1.0
        walls[..., :, -1] = 1.0
        pin = torch.zeros((1, 1, n, n))
        pin[..., 0, 0] = 1.0
        x = torch.linspace(0.0, 1.0, n)
        u_bc = torch.zeros((1, 1, n, n))
        u_bc[..., -1, :] = 1.0 - 16.0 * (x - 0.5) ** 4
        self.register_buffer("bc1", walls)
        self.register_buffer("bc2", walls.clone())
        self.register_buffer("bc3", pin)
        self.register_buffer("u_bc", u_bc)

    def fields(self):
        return self.net_u[0], self.net_v[0], self.net_p[0]

    def loss(self, stage="ns"):
        """(||R1||, ||R2||, ||R3||) -- e1_ns_ldc_resmin.py:310-313 (stage "ns") or the Stokes stage of the e2 scripts (stage "stokes")"""
        bc = (self.bc1, self.bc2, self.bc3)
        if stage == "stokes":
            kw = dict(bc_values=(self.u_bc, 0.0, 0.0), visco=self.viscosity, pspg=self.hx * self.hy * self.Re / 12.0, wscale=1.0)
            if self.mode == "fused":
                return stokes_loss(self, *self.fields(), bc, **kw)
            return tuple(torch.norm(R) for R in stokes_residuals_composed(self, *self.fields(), bc, **kw))
        kw = dict(bc_values=(self.u_bc, 0.0, 0.0), visco=self.viscosity)
        if self.mode == "fused":
            return ns_loss(self, *self.fields(), bc, **kw)
        return tuple(torch.norm(R) for R in ns_residuals_composed(self, *self.fields(), bc, **kw))


def run(size=64, steps=200, lr=5e-4, Re=100.0, mode="fused", stokes_steps=0, verbose=True, seed=42):
    """Trains and returns (model, history): history[i] = the three norms after the forward of step i (float64 numpy array per step); the
    first `stokes_steps` entries are Stokes-stage norms."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(seed)
    n = size
    mk = lambda: nn.ParameterList([nn.Parameter(0.1 * (torch.rand((1, 1, n, n), generator=g) - 0.5))])     # noqa: E731
    model = NSLDC((mk(), mk(), mk()), Re=Re, mode=mode, domain_size=n).to(dev)
    opts = [torch.optim.Adam(p.parameters(), lr=lr) for p in (model.net_u, model.net_v, model.net_p)]
    history = []
    t0 = time.perf_counter()
    for step in range(stokes_steps + steps):
        stage = "stokes" if step < stokes_steps else "ns"
        for k, opt in enumerate(opts):                 # Lightning's multiple-optimiser loop: optimiser k steps on loss_vals[k]
            opt.zero_grad(set_to_none=True)
            norms = model.loss(stage)
            if k == 0:
                history.append(torch.stack([x.detach() for x in norms]).double().cpu().numpy())
            norms[k].backward()
            opt.step()
        if verbose and (step % 25 == 0 or step == stokes_steps + steps - 1):
            h = history[-1]
            print(f"step {step:4d} ({stage:6s})  ||R1|| {h[0]:.6e}  ||R2|| {h[1]:.6e}  ||R3|| {h[2]:.6e}", flush=True)
    torch.cuda.synchronize()
    if verbose:
        u = model.net_u[0].detach()
        print(f"{stokes_steps} + {steps} steps ({mode}) in {time.perf_counter() - t0:.2f} s; u at the centre {float(u[0, 0, n // 2, n // 2]):.6e}")
    return model, history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=5e-4)
    ap.add_argument("--re", type=float, default=100.0)
    ap.add_argument("--stokes-steps", type=int, default=0)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    a = ap.parse_args()
    run(a.size, a.steps, a.lr, a.re, a.mode, a.stokes_steps)


if __name__ == "__main__":
    main()
