#!/usr/bin/env python3
"""Signed-distance field of a sphere from a point cloud on the unit cube, solved for the nodal field itself -- the set-up of the
reference's `examples/eiqonal/single_instance/05_3d_sphere_loss4.py` (loss4) without Lightning or a network:

    loss = || R ||_F + sum_p u(x_p)^2 + sum_p (grad u(x_p) . n_p - 1)^2
    R_a  = sum_g JxW ( tau u gradN_a . grad u + (1 + tau) N_a |grad u|^2 - N_a ),  the stabilised eikonal residual |grad u| = 1

with the points x_p on a sphere of radius 0.3 around the centre and n_p their outward normals.  The script's domain term (4 Gauss-point
evaluations, elementwise passes over (B, 8, G, nel, nel, nel) tensors, the assembly, the norm and the autograd backward through all of it)
is ONE launch forward and one backward (diffnet_amd.eikonal.eikonal_loss on a DiffNet3DFEM: dn_eikonal3d_apply); the two point terms
stay in torch.

    python examples/eikonal_3d.py [--n 33] [--tau 0.25] [--mode fused|composed] [--optimizer lbfgs|adam] [--steps 20]

--mode fused     the fused HIP operator (dn_eikonal3d_apply)
       composed  the same residual on the drop-in operators (gauss_pt_evaluation*, assemble)
It prints the error against the exact signed distance (the 2-norm of the nodal difference over n^1.5).
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
from DiffNet.DiffNetFEM import DiffNet3DFEM  # noqa: E402  (reference import path, MI355X implementation)
from diffnet_amd import eikonal as ek  # noqa: E402
from diffnet_amd.tables import Basis1D  # noqa: E402

RADIUS, NPTS = 0.3, 256


def sphere_points(npts):
    """npts points on the unit sphere, a Fibonacci spiral"""
    k = np.arange(npts) + 0.5
    z = 1.0 - 2.0 * k / npts
    phi = math.pi * (1.0 + math.sqrt(5.0)) * k
    r = np.sqrt(1.0 - z * z)
    return np.stack((r * np.cos(phi), r * np.sin(phi), z), 1)


class Eikonal3D(DiffNet3DFEM):
    """One nodal parameter; the point cloud as interpolation weights of u, u_x, u_y and u_z on the 8 nodes of each point's element."""

    def __init__(self, field, n, tau=0.25, mode="fused"):
        super().__init__(None, None, domain_size=n, nsd=3)
        self.net, self.tau, self.mode = field, float(tau), mode
        nrm = sphere_points(NPTS)
        pts = 0.5 + RADIUS * nrm
        he = self.hx
        e = np.minimum((pts / he).astype(np.int64), n - 2)
        xi = 2.0 * (pts - e * he) / he - 1.0               # (NPTS, 3) in the element's [-1, 1]^3
        b = Basis1D(1)
        Bv = [b.val(xi[:, d]) for d in range(3)]           # (2, NPTS) per axis
        Dv = [b.der(xi[:, d]) * 2.0 / he for d in range(3)]
        o = np.arange(2)
        idx = (((e[:, 2])[:, None, None, None] + o[None, :, None, None]) * n + (e[:, 1])[:, None, None, None] + o[None, None, :, None]) * n \
            + (e[:, 0])[:, None, None, None] + o[None, None, None, :]
        w = lambda fz, fy, fx: torch.from_numpy((fz.T[:, :, None, None] * fy.T[:, None, :, None] * fx.T[:, None, None, :])      # noqa: E731
                                                .reshape(NPTS, -1).astype(np.float32))
        self.register_buffer("pidx", torch.from_numpy(idx.reshape(NPTS, -1)))
        self.register_buffer("wN", w(Bv[2], Bv[1], Bv[0]))
        self.register_buffer("wX", w(Bv[2], Bv[1], Dv[0]))
        self.register_buffer("wY", w(Bv[2], Dv[1], Bv[0]))
        self.register_buffer("wZ", w(Dv[2], Bv[1], Bv[0]))
        self.register_buffer("normals", torch.from_numpy(nrm.astype(np.float32)))
        x = np.linspace(0.0, 1.0, n)
        r = np.sqrt((x[None, None, :] - 0.5) ** 2 + (x[None, :, None] - 0.5) ** 2 + (x[:, None, None] - 0.5) ** 2)
        self.register_buffer("u_exact", torch.from_numpy((r - RADIUS).astype(np.float32))[None, None].contiguous())

    def point_terms(self, u):
        up = u.reshape(-1)[self.pidx]                      # (NPTS, 8)
        val, ux, uy, uz = ((up * w).sum(1) for w in (self.wN, self.wX, self.wY, self.wZ))
        nr = self.normals
        return torch.sum(val ** 2) + torch.sum((ux * nr[:, 0] + uy * nr[:, 1] + uz * nr[:, 2] - 1.0) ** 2)

    def domain_term(self, u):
        if self.mode == "fused":
            return ek.eikonal_loss(self, u, kind="norm", **ek.eikonal_coefficients(self.tau))
        return torch.norm(ek.eikonal_residual_composed(self, u, **ek.eikonal_coefficients(self.tau)))

    def loss(self):
        u = self.net[0]
        return self.domain_term(u) + self.point_terms(u)

    def error(self):
        u = self.net[0].detach()
        return float(torch.linalg.vector_norm(u - self.u_exact)) / u.shape[-1] ** 1.5


def run(n=33, steps=20, optimizer="lbfgs", mode="fused", verbose=True, tau=0.25, lr=1e-2):
    if mode not in ("fused", "composed"):
        raise ValueError(f"mode must be 'fused' or 'composed', got {mode!r}")
    dev = torch.device("cuda")
    x = torch.linspace(0.0, 1.0, n)
    # start from a field with a minimum in the sphere's centre and the wrong slope: |grad u| = 0.4
    r = torch.sqrt((x[None, None, :] - 0.5) ** 2 + (x[None, :, None] - 0.5) ** 2 + (x[:, None, None] - 0.5) ** 2)
    u0 = 0.4 * (r - RADIUS)
    field = nn.ParameterList([nn.Parameter(u0.reshape(1, 1, n, n, n).contiguous().to(dev))])
    m = Eikonal3D(field, n, tau, mode).to(dev)
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
        print(f"{steps} steps in {time.perf_counter() - t0:.2f} s ({mode}, {optimizer}, {n}^3 nodes Q1, tau {tau}); final loss {hist[-1]:.6e}; "
              f"|| u - u_exact || / n^1.5 = {m.error():.4e}")
    return field[0].detach(), hist


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=33)
    ap.add_argument("--tau", type=float, default=0.25)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    ap.add_argument("--optimizer", choices=("lbfgs", "adam"), default="lbfgs")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lr", type=float, default=1e-2)
    a = ap.parse_args()
    run(a.n, a.steps, a.optimizer, a.mode, True, a.tau, a.lr)


if __name__ == "__main__":
    main()
