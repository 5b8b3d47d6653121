#!/usr/bin/env python3
"""Device time of the fused point-cloud terms (dn_points_apply) against their torch forms, HIP events:

  3-D   129^3 nodes x 10 242 points, B = 1     the setting of examples/eikonal_3d.py at full size (value term + "dot" normals term)
  2-D   512^2 nodes x 1 000 points, B = 16
  3-D   33^3 nodes x 1 000 points, B = 1       bound by launch overhead

Arms per case, all on the same field, cloud and normals:
  fused forward     one launch: values, both sums, the per-point cotangents
  fused adjoint     one launch: the dense gather over the nodes
  fused pair        points.point_loss_and_grad: both launches from one call
  composed forward  points.point_terms_composed with the autograd graph recorded
  composed pair     ... and its backward (ends in an index_put with accumulation)
  weights pair      3-D cases: the form examples/eikonal_3d.py had before the fused terms -- precomputed node indices and four weight
                    tables, `u.reshape(-1)[pidx]`, four weighted sums, two reductions -- forward and backward
  node write        a memset of the gradient (4 B nodes bytes): the write half of the adjoint's stream
and the time to build the PointPlan (host clock around the build and a synchronise; a fixed cloud pays it once).

Every arm is warmed up, then the arms are timed in rounds, one call of each arm per round; the figure is the median over the rounds with
the smallest and largest value as the spread.  An event pair around ONE call measures the call: where the host enqueues more slowly than
the device runs (every fused arm here; "node write" shows the floor of one enqueued call) it is host time.  Kernel times come from a run
of this tool under `rocprofv3 --kernel-trace --stats`, in a run of its own (profiles/point_terms.txt holds both).  The dense adjoint reads 4 B nel bytes of offsets and writes 4 B nodes
bytes however few points there are: its time is quoted beside that stream at 6.3 TB/s.

The one condition: in every case the fused pair is not slower than the composed pair (and, in 3-D, than the weights pair).  Exit
status 1 if it is.

    python tools/bench_points.py [--rounds 30] [--out profiles/point_terms.txt]
"""
import argparse
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffnet_amd import ops, points as pt  # noqa: E402
from diffnet_amd.fem import FemGeometry  # noqa: E402
from diffnet_amd.tables import gauss_rule  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_winding import fibonacci_sphere, time_arms  # noqa: E402

HBM = 6.3e12


def geometry(nodes):
    gx, gw = gauss_rule(2)
    return FemGeometry(len(nodes), nodes, tuple(1.0 / (n - 1) for n in nodes), 1, 2, gx, gw)


def weight_tables(geom, pts, dev):
    """the buffers of the earlier examples/eikonal_3d.py: node indices (P, 8) and the weights of u, u_x, u_y, u_z, from float64"""
    n, he = geom.sizes[0], geom.hs[0]
    p = pts.double().cpu()
    e = torch.clamp((p / he).long(), max=n - 2)
    xi = 2.0 * (p - e * he) / he - 1.0
    val = [torch.stack((0.5 * (1 - xi[:, d]), 0.5 * (1 + xi[:, d]))) for d in range(3)]
    der = [torch.stack((-0.5 * torch.ones_like(xi[:, d]), 0.5 * torch.ones_like(xi[:, d]))) * 2.0 / he for d in range(3)]
    o = torch.arange(2)
    idx = ((e[:, 2, None, None, None] + o[None, :, None, None]) * n + e[:, 1, None, None, None] + o[None, None, :, None]) * n \
        + e[:, 0, None, None, None] + o[None, None, None, :]
    w = lambda fz, fy, fx: (fz.T[:, :, None, None] * fy.T[:, None, :, None] * fx.T[:, None, None, :]).reshape(len(p), -1).float().to(dev)      # noqa: E731
    return idx.reshape(len(p), -1).to(dev), w(val[2], val[1], val[0]), w(val[2], val[1], der[0]), w(val[2], der[1], val[0]), w(der[2], val[1], val[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_terms.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines, ok = [], True
    g = torch.Generator().manual_seed(0)
    unit = fibonacci_sphere(10242)
    th = torch.rand((16, 1000), generator=g) * 2 * math.pi
    circle = torch.stack((torch.cos(th), torch.sin(th)), -1)
    cases = (("3-D 129^3 x 10242 pts x B=1", (129, 129, 129), unit[None]),
             ("2-D 512^2 x 1000 pts x B=16", (512, 512), circle),
             ("3-D 33^3 x 1000 pts x B=1", (33, 33, 33), fibonacci_sphere(1000)[None]))
    for title, nodes, nrm in cases:
        geom = geometry(nodes)
        B, P, nsd = nrm.shape[0], nrm.shape[1], len(nodes)
        pts = (0.5 + 0.3 * nrm).to(dev).contiguous()
        nrm = nrm.to(dev).contiguous()
        u = torch.randn((B, 1, *geom.node_shape), generator=g).to(dev)
        torch.cuda.synchronize()
        builds = []
        for _ in range(5):
            t0 = time.perf_counter()
            plan = pt.PointPlan(geom, pts)
            torch.cuda.synchronize()
            builds.append((time.perf_counter() - t0) * 1e6)
        kw = dict(target=0.0, normals=nrm, kind="dot", dscale="physical")
        skw = dict(dscale=plan.dscale("physical"), kind="dot", normals=plan.sort(nrm, vector=True))
        _, _, _, cot, _ = ops.points_apply(geom, B, P, plan.xi, plan.elem, u=u, penalty=True, want_cot=True, **skw)
        grad = torch.empty_like(u)
        ur = u.clone().requires_grad_(True)

        def composed_pair():
            ur.grad = None
            pt.point_terms_composed(geom, ur, plan, **kw).backward()

        arms = {"fused forward": lambda: ops.points_apply(geom, B, P, plan.xi, plan.elem, u=u, penalty=True, want_sums=True, want_cot=True, **skw),
                "fused adjoint": lambda: ops.points_apply(geom, B, P, plan.xi, offsets=plan.offsets, dscale=skw["dscale"], cot=cot, want_grad=True, grad_out=grad),
                "fused pair": lambda: pt.point_loss_and_grad(geom, u, plan, grad_out=grad, **kw),
                "composed forward": lambda: pt.point_terms_composed(geom, ur, plan, **kw),
                "composed pair": composed_pair,
                "node write": lambda: grad.zero_()}
        if nsd == 3:
            pidx, wN, wX, wY, wZ = weight_tables(geom, pts[0], dev)

            def weights_pair():
                ur.grad = None
                up = ur.reshape(-1)[pidx]
                val, ux, uy, uz = ((up * w).sum(1) for w in (wN, wX, wY, wZ))
                (torch.sum(val ** 2) + torch.sum((ux * nrm[0, :, 0] + uy * nrm[0, :, 1] + uz * nrm[0, :, 2] - 1.0) ** 2)).backward()

            arms["weights pair"] = weights_pair
        t = time_arms(arms, a.rounds)
        for k, v in t.items():
            lines.append(f"{title:30s} {k:18s} {v[len(v) // 2]:9.1f} us (min {v[0]:.1f}, max {v[-1]:.1f}; {len(v)} rounds)")
            print(lines[-1], flush=True)
        med = {k: v[len(v) // 2] for k, v in t.items()}
        builds.sort()
        stream = 4.0 * B * (geom.nelem_total + geom.nnode_total)
        lines.append(f"{title:30s} plan build         {builds[len(builds) // 2]:9.1f} us host clock with a synchronise (min {builds[0]:.1f}, max {builds[-1]:.1f}; 5 builds)")
        lines.append(f"{title:30s} adjoint stream: {stream / 1e6:.2f} MB of offsets and nodes = {stream / HBM * 1e6:.2f} us at 6.3 TB/s; measured {med['fused adjoint']:.1f} us")
        others = [k for k in ("composed pair", "weights pair") if k in med]
        for k in others:
            met = med["fused pair"] <= med[k]
            ok = ok and met
            lines.append(f"{title:30s} condition: fused pair {med['fused pair']:.1f} us <= {k} {med[k]:.1f} us ({med[k] / med['fused pair']:.1f} x): {'met' if met else 'NOT met'}")
        for ln in lines[-2 - len(others):]:
            print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("tools/bench_points.py: HIP-event times, median over rounds in which the arms alternate (spread: min, max)\n")
        fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
