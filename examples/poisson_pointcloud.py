#!/usr/bin/env python3
"""Poisson problem with its boundary condition given as a point cloud, solved for the nodal field itself -- the set-up of the reference's
`examples/poisson/single_instance/pc_poisson_disk.py` (and `pc_complex_immersed_background.py`) without Lightning or a network:

    loss = mean_e sum_g w_g ( |grad u|^2 - u f ) + sum_p ( u(x_p) - 1 )^2,        f = 1

with the points x_p on a circle of radius 0.25 around the centre of the unit square: the penalty pins u to 1 on the circle, the energy
term solves -2 lap u = f around it.  The energy term is ONE launch forward and one backward (DiffNet2DFEM.energy_loss); so is the point
term (diffnet_amd.points.point_loss on a `PointPlan`), which in the script is four gathers, the products of the 1-D bases, two sums, a
square and a reduction, and an index_put with accumulation on the way back.

    python examples/poisson_pointcloud.py [--n 65] [--npts 200] [--points fused|composed] [--axes physical|transposed] [--steps 30]

--points fused       the fused point term (dn_points_apply)
         composed    the same term in plain torch ops (points.point_terms_composed)
--axes transposed    the scripts' `u[b, 0, nidx, nidy]`: x indexes rows (on this symmetric problem the field comes out transposed)
It prints the loss, the largest |u(x_p) - 1| over the cloud and the field's value in the centre of the circle.
"""
import argparse
import math
import os
import sys
import time

import torch
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from DiffNet.DiffNetFEM import DiffNet2DFEM  # noqa: E402  (reference import path, MI355X implementation)
from diffnet_amd import points as pt  # noqa: E402

RADIUS = 0.25


class PointCloudPoisson(DiffNet2DFEM):
    """One nodal parameter, the forcing f = 1 and the cloud as a `PointPlan` of the mesh."""

    def __init__(self, field, n, npts=200, points="fused", axes=None):
        super().__init__(None, None, domain_size=n)
        self.net, self.points, self.axes = field, points, axes
        t = 2.0 * math.pi * (torch.arange(npts, dtype=torch.float64) + 0.5) / npts
        self.register_buffer("pts", (0.5 + RADIUS * torch.stack((torch.cos(t), torch.sin(t)), 1)).float()[None].contiguous())       # (1, npts, 2)
        self.register_buffer("f", torch.ones(1, 1, n, n))
        self.plan = None                                   # the cloud is fixed: classified and sorted once, on the field's device

    def point_term(self, u):
        if self.plan is None or self.plan.device != u.device:
            self.plan = pt.PointPlan(self, self.pts, axes=self.axes)
        terms = pt.point_loss if self.points == "fused" else pt.point_terms_composed
        return terms(self, u, self.plan, target=1.0)

    def loss(self):
        u = self.net[0]
        return self.energy_loss(u, f=self.f, c=1.0) + self.point_term(u)

    def report(self):
        u = self.net[0].detach()
        vals, _ = pt.eval_at_points(self, u, self.plan)
        return float((vals - 1.0).abs().max()), float(u[0, 0, u.shape[2] // 2, u.shape[3] // 2])


def run(n=65, npts=200, steps=30, points="fused", axes="physical", verbose=True):
    if points not in ("fused", "composed") or axes not in ("physical", "transposed"):
        raise ValueError(f"points must be 'fused' or 'composed' and axes 'physical' or 'transposed', got {points!r}, {axes!r}")
    dev = torch.device("cuda")
    field = nn.ParameterList([nn.Parameter(torch.zeros(1, 1, n, n, device=dev))])
    m = PointCloudPoisson(field, n, npts, points, None if axes == "physical" else axes).to(dev)
    opt = torch.optim.LBFGS(field, lr=1.0, max_iter=20, history_size=20, line_search_fn="strong_wolfe")
    hist = []

    def closure():
        opt.zero_grad(set_to_none=True)
        val = m.loss()
        val.backward()
        return val

    t0 = time.perf_counter()
    for it in range(steps):
        hist.append(float(opt.step(closure).detach()))
        if verbose:
            print(f"step {it:4d}  loss {hist[-1]:.6e}")
    with torch.no_grad():
        hist.append(float(m.loss()))
    torch.cuda.synchronize()
    dev_max, centre = m.report()
    if verbose:
        print(f"{steps} L-BFGS steps in {time.perf_counter() - t0:.2f} s (points {points}, axes {axes}, {n}^2 nodes, {npts} points); final loss {hist[-1]:.6e}; "
              f"max |u(x_p) - 1| = {dev_max:.3e}; u(centre) = {centre:.4e}")
    return field[0].detach(), hist


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=65)
    ap.add_argument("--npts", type=int, default=200)
    ap.add_argument("--points", choices=("fused", "composed"), default="fused")
    ap.add_argument("--axes", choices=("physical", "transposed"), default="physical")
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    run(a.n, a.npts, a.steps, a.points, a.axes)


if __name__ == "__main__":
    main()
