#!/usr/bin/env python3
"""Immersed-boundary Poisson problem around a 3-D object given as an oriented point cloud, solved for the nodal field itself -- the
flow of the reference's IBN/poisson-3d/non-parametric/solve_in_object_3d.py (object mask -> Dirichlet source, box faces -> sink,
energy loss on a bare nodal parameter) with the object coming from points, normals and areas, as in
examples/eiqonal/single_instance/02_differentiable_winding_number.py, instead of a voxel file:

    cloud (N, 3) + normals + areas  --winding_mask (one HIP launch, dn_winding_field)-->  uint8 inside mask on the mesh nodes
    u = 1 on the mask, u = 0 on the six box faces,  minimise  mean_e sum_g w_g (1/2) |grad u|^2   (dn_poisson_apply, fused, 3-D Q1)

    python examples/ibn_3d_pointcloud.py [--n 33] [--shape sphere|ellipsoid] [--points 2000] [--xyzna FILE] [--steps 30] [--optimizer lbfgs|adam]

--xyzna FILE reads a cloud in the reference's text format (count, points, normals, areas); it is scaled and centred into the unit cube
(longest extent 0.6).  The winding number is not differentiated: only its mask is used, as in the reference.
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
from diffnet_amd.ops import BoxFaces  # noqa: E402
from diffnet_amd.winding import read_xyzna, winding_mask  # noqa: E402


def fibonacci_sphere(npts):
    """npts points on the unit sphere, a Fibonacci spiral"""
    k = np.arange(npts) + 0.5
    z = 1.0 - 2.0 * k / npts
    phi = math.pi * (1.0 + math.sqrt(5.0)) * k
    r = np.sqrt(1.0 - z * z)
    return np.stack((r * np.cos(phi), r * np.sin(phi), z), 1)


def ellipsoid_cloud(npts, axes, centre=(0.5, 0.5, 0.5)):
    """points, unit normals and areas of an ellipsoid: the Fibonacci sphere mapped by x -> centre + axes * x.  A patch of the sphere with
    normal s and area dA maps to one with normal ~ s / axes and area dA * a b c |s / axes|."""
    s = fibonacci_sphere(npts)
    ax = np.asarray(axes, dtype=np.float64)
    g = s / ax
    gn = np.linalg.norm(g, axis=1, keepdims=True)
    area = (4.0 * math.pi / npts) * ax.prod() * gn
    return np.asarray(centre) + ax * s, g / gn, area


def load_cloud(path):
    pts, nrm, area = read_xyzna(path)
    lo, hi = pts.min(0), pts.max(0)
    s = 0.6 / float((hi - lo).max())
    return 0.5 + s * (pts - 0.5 * (lo + hi)), nrm / np.linalg.norm(nrm, axis=1, keepdims=True), area * s * s


class ObjectPoisson(DiffNet3DFEM):
    def __init__(self, field, source, n):
        super().__init__(None, None, domain_size=n, nsd=3)
        self.net = field
        self.source = source                               # uint8 (1, 1, n, n, n), straight from the winding kernel
        self.sink = BoxFaces("all")

    def loss(self):
        return self.energy_loss(self.net[0], None, None, dirichlet=[(self.source, 1.0), (self.sink, 0.0)], c=0.5)


def run(n=33, shape="sphere", npts=2000, xyzna=None, steps=30, optimizer="lbfgs", verbose=True, lr=5e-2):
    dev = torch.device("cuda")
    if xyzna:
        pts, nrm, area = load_cloud(xyzna)
        volume = None
    else:
        axes = {"sphere": (0.3, 0.3, 0.3), "ellipsoid": (0.34, 0.22, 0.16)}[shape]
        pts, nrm, area = ellipsoid_cloud(npts, axes)
        volume = 4.0 / 3.0 * math.pi * float(np.prod(axes))
    m0 = DiffNet3DFEM(None, None, domain_size=n, nsd=3)
    nodes = torch.stack((m0.xx, m0.yy, m0.zz)).to(dev)         # (3, n, n, n): the kernel's coordinate-major query list, no copy
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None].to(dev)      # noqa: E731
    t0 = time.perf_counter()
    source = winding_mask(f32(pts), f32(nrm), f32(area), nodes)
    torch.cuda.synchronize()
    t_mask = time.perf_counter() - t0
    frac = float(source.float().mean())
    if verbose:
        exact = "" if volume is None else f" (the object's volume: {volume:.4f})"
        print(f"winding mask of {pts.shape[0]} points on {n}^3 nodes: {int(source.sum())} nodes inside, node fraction {frac:.4f}{exact}; "
              f"{t_mask * 1e3:.1f} ms with the first-call set-up")
    if source[:, :, [0, -1]].any() or source[:, :, :, [0, -1]].any() or source[..., [0, -1]].any():
        raise ValueError("the object touches the box faces: source and sink conditions would overlap")
    field = nn.ParameterList([nn.Parameter(torch.zeros(1, 1, n, n, n, device=dev))])
    model = ObjectPoisson(field, source, n).to(dev)
    if optimizer == "lbfgs":
        opt = torch.optim.LBFGS(field, lr=1.0, max_iter=10, history_size=20, line_search_fn="strong_wolfe")
    elif optimizer == "adam":
        opt = torch.optim.Adam(field, lr=lr)
    else:
        raise ValueError(f"optimizer must be 'lbfgs' or 'adam', got {optimizer!r}")
    hist = []

    def closure():
        opt.zero_grad(set_to_none=True)
        val = model.loss()
        val.backward()
        return val

    t0 = time.perf_counter()
    for it in range(steps):
        hist.append(float(opt.step(closure).detach()))
        if verbose and (it % 5 == 0 or it == steps - 1):
            print(f"step {it:4d}  energy {hist[-1]:.6e}")
    with torch.no_grad():
        hist.append(float(model.loss()))
        u = torch.where(source > 0, torch.ones_like(field[0]), field[0])
        for ax in (2, 3, 4):                               # the conditions as the loss applies them
            u.select(ax, 0).zero_()
            u.select(ax, n - 1).zero_()
    torch.cuda.synchronize()
    if verbose:
        print(f"{steps} steps in {time.perf_counter() - t0:.2f} s ({optimizer}, {n}^3 nodes Q1); energy {hist[0]:.6e} -> {hist[-1]:.6e}; "
              f"u in [{float(u.min()):.3f}, {float(u.max()):.3f}], mean {float(u.mean()):.4f}")
    return u, hist, source


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=33)
    ap.add_argument("--shape", choices=("sphere", "ellipsoid"), default="sphere")
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--xyzna", default=None)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--optimizer", choices=("lbfgs", "adam"), default="lbfgs")
    ap.add_argument("--lr", type=float, default=5e-2)
    a = ap.parse_args()
    run(a.n, a.shape, a.points, a.xyzna, a.steps, a.optimizer, True, a.lr)


if __name__ == "__main__":
    main()
