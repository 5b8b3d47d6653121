#!/usr/bin/env python3
"""Signed-distance field of a circle from a point cloud on the unit square, solved for the nodal field itself -- the set-up of the
reference's `examples/eiqonal/single_instance/e01_curve_reconstruction.py` (loss4) and `examples/eiqonal/parametric/10_fixed_bc.py`
(loss_eikonal) without Lightning, NURBS or a network:

    loss = || R ||_F + sum_p u(x_p)^2 + sum_p (grad u(x_p) . n_p - 1)^2
    R_a  = sum_g JxW ( tau u gradN_a . grad u + (1 + tau) N_a |grad u|^2 - N_a ),  the stabilised eikonal residual |grad u| = 1

with the points x_p on a circle of radius 0.3 around the centre and n_p their outward normals.  The scripts' domain term (3 Gauss-point
evaluations, elementwise passes over (B, nbf, G, nel, nel) tensors, the assembly, the norm and the autograd backward through all of it) is
ONE launch forward and one backward (diffnet_amd.eikonal.eikonal_loss); the two point terms -- an index gather, three weighted sums, two
reductions and their autograd replay -- are one launch forward and one backward too (diffnet_amd.points.point_loss on a `PointPlan`).

    python examples/eikonal_2d.py [--n 65] [--degree 1] [--tau 0.25] [--mode fused|composed] [--points fused|composed]
                                  [--optimizer lbfgs|adam] [--steps 20]

--mode fused       the fused HIP operator (dn_eikonal_apply)
       composed    the same residual on the drop-in operators (gauss_pt_evaluation*, assemble)
--points fused     the fused point terms (dn_points_apply; Q1 meshes: on a Q2 / Q3 mesh point_loss composes torch ops itself)
         composed  the same terms in plain torch ops (points.point_terms_composed)
It prints the error against the exact signed distance (the 2-norm of the nodal difference over n).
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
from diffnet_amd import eikonal as ek  # noqa: E402
from diffnet_amd import points as pt  # noqa: E402

RADIUS, NPTS = 0.3, 64


class Eikonal(DiffNet2DFEM):
    """One nodal parameter; the point cloud as a `PointPlan` of the mesh."""

    def __init__(self, field, n, degree=1, tau=0.25, mode="fused", points="fused"):
        super().__init__(None, None, domain_size=n, fem_basis_deg=degree)
        self.net, self.tau, self.mode, self.points = field, float(tau), mode, points
        t = 2.0 * math.pi * (np.arange(NPTS) + 0.5) / NPTS
        nrm = np.stack((np.cos(t), np.sin(t)), 1)
        self.register_buffer("pts", torch.from_numpy((0.5 + RADIUS * nrm).astype(np.float32))[None].contiguous())       # (1, NPTS, 2)
        self.register_buffer("normals", torch.from_numpy(nrm.astype(np.float32))[None].contiguous())
        self.plan = None                                   # the cloud is fixed: classified and sorted once, on the field's device
        x = np.linspace(0.0, 1.0, n)
        xx, yy = np.meshgrid(x, x)
        self.register_buffer("u_exact", torch.from_numpy((np.hypot(xx - 0.5, yy - 0.5) - RADIUS).astype(np.float32))[None, None].contiguous())

    def point_terms(self, u):
        if self.plan is None or self.plan.device != u.device:
            self.plan = pt.PointPlan(self, self.pts)
        terms = pt.point_loss if self.points == "fused" else pt.point_terms_composed
        return terms(self, u, self.plan, target=0.0, normals=self.normals, kind="dot", dscale="physical")

    def domain_term(self, u):
        if self.mode == "fused":
            return ek.eikonal_loss(self, u, kind="norm", **ek.eikonal_coefficients(self.tau))
        return torch.norm(ek.eikonal_residual_composed(self, u, **ek.eikonal_coefficients(self.tau)))

    def loss(self):
        u = self.net[0]
        return self.domain_term(u) + self.point_terms(u)

    def error(self):
        u = self.net[0].detach()
        return float(torch.linalg.vector_norm(u - self.u_exact)) / u.shape[-1]


def run(n=65, degree=1, tau=0.25, steps=20, optimizer="lbfgs", mode="fused", lr=1e-2, verbose=True, points="fused"):
    if mode not in ("fused", "composed") or points not in ("fused", "composed"):
        raise ValueError(f"mode and points must be 'fused' or 'composed', got {mode!r}, {points!r}")
    if (n - 1) % degree:
        raise ValueError(f"degree-{degree} elements need (n - 1) % {degree} == 0 nodes per axis")
    dev = torch.device("cuda")
    x = torch.linspace(0.0, 1.0, n)
    # start from a field with a minimum inside the circle's centre and the wrong slope: |grad u| = 0.4
    u0 = 0.4 * (torch.hypot(x[None, :] - 0.5, x[:, None] - 0.5) - RADIUS)
    field = nn.ParameterList([nn.Parameter(u0.reshape(1, 1, n, n).contiguous().to(dev))])
    m = Eikonal(field, n, degree, tau, mode, points).to(dev)
    if optimizer == "lbfgs":
        opt = torch.optim.LBFGS(field, lr=1.0, max_iter=5)
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
            print(f"step {it:4d}  loss {hist[-1]:.6e}  error of u {m.error():.4e}")
    with torch.no_grad():
        hist.append(float(m.loss()))
    torch.cuda.synchronize()
    if verbose:
        print(f"{steps} steps in {time.perf_counter() - t0:.2f} s ({mode}, points {points}, {optimizer}, {n}^2 nodes Q{degree}, tau {tau}); final loss {hist[-1]:.6e}; "
              f"|| u - u_exact || / n = {m.error():.4e}")
    return field[0].detach(), hist


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=65)
    ap.add_argument("--degree", type=int, default=1)
    ap.add_argument("--tau", type=float, default=0.25)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    ap.add_argument("--points", choices=("fused", "composed"), default="fused")
    ap.add_argument("--optimizer", choices=("lbfgs", "adam"), default="lbfgs")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lr", type=float, default=1e-2)
    a = ap.parse_args()
    run(a.n, a.degree, a.tau, a.steps, a.optimizer, a.mode, a.lr, points=a.points)


if __name__ == "__main__":
    main()
