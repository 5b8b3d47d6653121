#!/usr/bin/env python3
"""Scalar transport on the unit square by minimising the sum of squares of the SUPG-stabilised weak-form residual over the nodal field u
-- the set-ups of three scripts of the reference under `examples/poisson/single_instance/`, on the ported datasets, without Lightning:

    --case advdiff    e17_adv_diff_2d_resmin.py: steady advection-diffusion, a = (cos pi/6, sin pi/6), AdvDiff2dRectangle (u = 1 / u = 0 faces)
           stheat     e3_st_mms_resmin.py: space-time heat (y is time), SUPG in time, SpaceTimeRectangleManufactured (u0 on the first row)
           allencahn  e18_allen_cahn_ice_melt.py: space-time Allen-Cahn with the cubic reaction, AllenCahnIceMeltRectangle

The scripts' loss body (3-4 Gauss-point evaluations, ~25 elementwise passes, a sliced assembly, two `where`s on u and two on R) is ONE
launch (diffnet_amd.transport.transport_loss), its backward another.

    python examples/transport_2d.py [--case advdiff] [--size 64] [--steps 200] [--lr 1e-2] [--mode fused|composed]

--mode fused     transport_loss: the fused HIP operator
       composed  transport_residual_composed + torch.sum: the same residual on the drop-in operators (gauss_pt_evaluation*, assemble)
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
from DiffNet.datasets.single_instances.rectangles import (AdvDiff2dRectangle, AllenCahnIceMeltRectangle,  # noqa: E402
                                                          SpaceTimeRectangleManufactured)
from diffnet_amd.transport import (advdiff_coefficients, allen_cahn_coefficients, space_time_heat_coefficients, transport_loss,  # noqa: E402
                                   transport_residual_composed)


class Transport2D(DiffNet2DFEM):
    """The scripts' modules in their `no_network` mode: one nodal parameter field, the dataset's two masks, the case's coefficients."""

    def __init__(self, field, dataset, case, mode="fused", **kwargs):
        super().__init__(None, dataset, **kwargs)
        self.net_u, self.mode = field, mode
        inp, _ = dataset[0]
        inp = torch.as_tensor(np.asarray(inp), dtype=torch.float32)
        self.register_buffer("bc1", inp[None, 1:2].contiguous())
        self.register_buffer("bc2", inp[None, 2:3].contiguous())
        if case == "advdiff":
            self.register_buffer("nu", inp[None, 0:1].contiguous())
            self.coef, self.first, v1 = advdiff_coefficients(self, (math.cos(math.pi / 6), math.sin(math.pi / 6)), 1e-4), False, None
        elif case == "stheat":
            self.nu = None
            self.coef, self.first, v1 = space_time_heat_coefficients(self, dataset.diffusivity), True, dataset.u0
        else:
            self.nu = None
            self.coef, self.first = allen_cahn_coefficients(dataset.ac_A, dataset.ac_Cn, dataset.ac_D, dataset.ac_k), False
            v1 = dataset.u0
        if v1 is None:
            self.v1 = 1.0
        else:
            self.register_buffer("v1", torch.as_tensor(np.asarray(v1), dtype=torch.float32)[None, None].contiguous())

    def loss(self):
        adv, kappa, tau, react = self.coef
        kw = dict(bc=(self.bc1, self.bc2), bc_values=(self.v1, 0.0), nu=self.nu, adv=adv, kappa=kappa, tau=tau, react=react,
                  r_first_wins=self.first)
        if self.mode == "fused":
            return transport_loss(self, self.net_u[0], **kw)
        return torch.sum(transport_residual_composed(self, self.net_u[0], **kw) ** 2)


DATASETS = dict(advdiff=AdvDiff2dRectangle, stheat=SpaceTimeRectangleManufactured, allencahn=AllenCahnIceMeltRectangle)


def run(case="advdiff", size=64, steps=200, lr=1e-2, mode="fused", verbose=True, seed=42):
    """Trains and returns (model, history): history[i] = the loss after the forward of step i."""
    dev = torch.device("cuda", 0)
    np.random.seed(seed)
    g = torch.Generator().manual_seed(seed)
    ds = DATASETS[case](domain_size=size)
    init = getattr(ds, "initial_guess", None)
    u0 = torch.as_tensor(np.asarray(init), dtype=torch.float32) if init is not None else 0.1 * torch.rand((size, size), generator=g)
    field = nn.ParameterList([nn.Parameter(u0.reshape(1, 1, size, size).clone())])
    model = Transport2D(field, ds, case, mode=mode, domain_size=size).to(dev)
    opt = torch.optim.Adam(model.net_u.parameters(), lr=lr)
    history = []
    t0 = time.perf_counter()
    for step in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = model.loss()
        history.append(float(loss.detach()))
        loss.backward()
        opt.step()
        if verbose and (step % 25 == 0 or step == steps - 1):
            print(f"step {step:4d}  sum R^2 {history[-1]:.6e}", flush=True)
    torch.cuda.synchronize()
    if verbose:
        u = model.net_u[0].detach()
        print(f"{case}: {steps} steps ({mode}) in {time.perf_counter() - t0:.2f} s; u at the centre {float(u[0, 0, size // 2, size // 2]):.6e}")
    return model, history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=tuple(DATASETS), default="advdiff")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    a = ap.parse_args()
    run(a.case, a.size, a.steps, a.lr, a.mode)


if __name__ == "__main__":
    main()
