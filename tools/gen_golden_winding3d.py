#!/usr/bin/env python3
"""Golden vectors of the 3-D winding-number field from the *imported* reference function.

Like tools/gen_golden_eikonal3d.py (whose shims it reuses), this runs only where the reference repository is present.  It imports
examples/eiqonal/single_instance/02_differentiable_winding_number.py as a module (matplotlib in its Agg backend, trimesh stubbed; the
script's own xyzna_reader and vis_linspecer import from its directory) and calls its `compute_winding_torch` on the CPU, once in float64
and once in float32.  Only data -- inputs and the reference's outputs -- is written:

  tests/golden/winding3d_n5_p37.npz      a 5^3 probe grid on [-0.5, 0.5]^3 (the script's own meshgrid, "ij" order), B = 2 clouds of 37 points
                                          on two spheres of different radius and centre, areas that differ between the samples and per point
  tests/golden/PROVENANCE_winding3d.txt

The file holds: script, q (1, 3, 5, 5, 5) float32, points / normals (2, 37, 3) float32, area (2, 37, 1) float32, winding64 (the reference on
the float32 inputs cast to float64) and winding32 (the reference in float32), both (1, 2, 5, 5, 5), and l1min, the smallest L1 distance
between a point and a probe (the generator asserts it is at least 1e-3: no probe sits on the cloud).

Usage: python tools/gen_golden_winding3d.py [--out tests/golden]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import T, install_shims, load_script, rng  # noqa: E402

SCRIPT = "examples/eiqonal/single_instance/02_differentiable_winding_number.py"

PROVENANCE = """winding3d_n5_p37.npz: written by tools/gen_golden_winding3d.py from the reference's own function, imported and called on the CPU:
  examples/eiqonal/single_instance/02_differentiable_winding_number.py::compute_winding_torch
Data only: a 5^3 probe grid on [-0.5, 0.5]^3 built as the script builds it, two clouds of 37 points on spheres (radius 0.31 about
(0.02, -0.03, 0.01) and radius 0.22 about (-0.05, 0.04, 0.03)) with unit normals and seeded areas, and the reference's result on them
in float64 (winding64) and float32 (winding32), (1, 2, 5, 5, 5) with the first two grid axes swapped as the reference returns them.
"""


def sphere(npts, g):
    z = 2.0 * torch.rand(npts, generator=g) - 1.0
    ph = 2.0 * math.pi * torch.rand(npts, generator=g)
    r = torch.sqrt(1.0 - z * z)
    return torch.stack((r * torch.cos(ph), r * torch.sin(ph), z), 1)


def gen(outdir):
    mod = load_script(SCRIPT, "ref_winding3d")
    n, npts = 5, 37
    q_0 = torch.linspace(-0.5, 0.5, n)
    qxx, qyy, qzz = torch.meshgrid(q_0, q_0, q_0, indexing="ij")               # what the script's torch.meshgrid call gives
    q = torch.stack((qxx, qyy, qzz), 0).unsqueeze(0)
    g = rng(41)
    pts, nrm, area = [], [], []
    for radius, centre, amp in ((0.31, (0.02, -0.03, 0.01), 1.0), (0.22, (-0.05, 0.04, 0.03), 0.6)):
        u = sphere(npts, g)
        pts.append(torch.tensor(centre) + radius * u)
        nrm.append(u)
        area.append(amp * 4.0 * math.pi * radius ** 2 / npts * (0.5 + torch.rand(npts, 1, generator=g)))
    pts, nrm, area = (torch.stack(v).float() for v in (pts, nrm, area))
    l1min = float((pts.double()[:, None] - q.double()[0].reshape(3, -1).T[None, :, None]).abs().sum(-1).min())
    assert l1min >= 1e-3, l1min
    w64 = mod.compute_winding_torch(pts.double(), nrm.double(), area.double(), q.double())
    w32 = mod.compute_winding_torch(pts, nrm, area, q)
    assert tuple(w64.shape) == (1, 2, n, n, n) and w64.dtype == torch.float64 and w32.dtype == torch.float32
    np.savez_compressed(os.path.join(outdir, "winding3d_n5_p37.npz"), script=SCRIPT + "::compute_winding_torch", q=T(q), points=T(pts),
                        normals=T(nrm), area=T(area), winding64=T(w64), winding32=T(w32), l1min=np.float64(l1min))
    with open(os.path.join(outdir, "PROVENANCE_winding3d.txt"), "w") as fh:
        fh.write(PROVENANCE)
    print("winding3d n5_p37", tuple(w64.shape), "max |w|", float(w64.abs().max()), "l1min", l1min,
          "max |w32 - w64|", float((w32.double() - w64).abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    a = ap.parse_args()
    install_shims()
    gen(a.out)


if __name__ == "__main__":
    main()
