#!/usr/bin/env python3
"""Fit the normals and areas of a point cloud to an occupancy field through the gradient of the winding number.

The points are a Fibonacci sphere (radius 0.3 about the centre of the unit cube).  The target is the true winding number of the true
normals and equal areas 4 pi r^2 / N on the n^3 nodes of the unit cube.  The fit starts from normals perturbed by 0.5 (U - 0.5) per
component and renormalised, and from areas at 0.6 x the truth, parameterised as exp(log a); Adam (lr 0.05) minimises
mean((w - target)^2).

    --mode fused      w = winding_number(..., differentiable=True): forward and backward are one HIP launch each (GPU only)
    --mode composed   w = winding_field_composed(...): the same sum in plain torch and its autograd graph (GPU or CPU)

    python examples/winding_fit.py [--mode fused|composed] [--n 17] [--points 1000] [--steps 100]

At --points 400 --n 9 --steps 60 the loss falls from 1.346e-2 to 1.564e-5 (a factor of 861) in both modes.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffnet_amd.winding import winding_field_composed, winding_number  # noqa: E402

RADIUS = 0.3


def fibonacci_sphere(npts):
    k = torch.arange(npts, dtype=torch.float64) + 0.5
    z = 1.0 - 2.0 * k / npts
    phi = math.pi * (1.0 + math.sqrt(5.0)) * k
    r = torch.sqrt(1.0 - z * z)
    return torch.stack((r * torch.cos(phi), r * torch.sin(phi), z), 1)


def run(mode="fused", n=17, npts=1000, steps=100, device=None, dtype=torch.float32, verbose=True):
    """Returns the list of losses, one per step (the loss before the step's update)."""
    if mode not in ("fused", "composed"):
        raise ValueError(f"mode must be 'fused' or 'composed', got {mode!r}")
    if device is None:
        device = torch.device("cuda:0" if mode == "fused" or torch.cuda.is_available() else "cpu")
    unit = fibonacci_sphere(npts)
    pts = (0.5 + RADIUS * unit).to(dtype)[None].contiguous().to(device)
    true_n = unit.to(dtype)[None].contiguous().to(device)
    true_a = torch.full((1, npts), 4.0 * math.pi * RADIUS ** 2 / npts, dtype=dtype, device=device)
    x = torch.linspace(0.0, 1.0, n, dtype=dtype)
    zz, yy, xx = torch.meshgrid(x, x, x, indexing="ij")
    q = torch.stack((xx, yy, zz)).contiguous().to(device)

    def field(normals, area):
        if mode == "fused":
            return winding_number(pts, normals, area, q, differentiable=True)
        return winding_field_composed(pts, normals, area, q, "l2", 3, 1.0 / (4.0 * math.pi)).reshape(1, 1, n, n, n)

    with torch.no_grad():
        target = field(true_n, true_a)
    g = torch.Generator().manual_seed(0)
    start = unit + 0.5 * (torch.rand((npts, 3), generator=g, dtype=torch.float64) - 0.5)
    start = start / torch.linalg.vector_norm(start, dim=-1, keepdim=True)
    normals = start.to(dtype)[None].contiguous().to(device).requires_grad_(True)
    log_a = torch.log(0.6 * true_a).requires_grad_(True)
    opt = torch.optim.Adam([normals, log_a], lr=0.05)
    hist = []
    for step in range(steps):
        opt.zero_grad()
        loss = ((field(normals, torch.exp(log_a)) - target) ** 2).mean()
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
        if verbose and (step % 10 == 0 or step == steps - 1):
            print(f"step {step:4d}  loss {hist[-1]:.4e}", flush=True)
    if verbose:
        print(f"mode {mode}, {npts} points, {n}^3 nodes, {steps} steps on {device}: first loss {hist[0]:.4e}, last loss {hist[-1]:.4e}, "
              f"ratio {hist[0] / hist[-1]:.1f}")
    return hist


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    ap.add_argument("--n", type=int, default=17)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=100)
    a = ap.parse_args()
    run(a.mode, a.n, a.points, a.steps)


if __name__ == "__main__":
    main()
