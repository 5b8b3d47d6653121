#!/usr/bin/env python3
"""Device time of the winding-number VJP (dn_winding_field_vjp, all three outputs), HIP events, in G point-query pairs per second, at

  probes   25^3 probes x 10 242 points, B = 1 (3-D, L1, cubed, area: compute_winding_torch's form), slices 1, 4, 16, 64 and automatic
  mesh     128^3 nodes x 10 242 points, B = 1 (the same form), slices 64, 256, 1024 and automatic
  2-D      64^2 nodes x 1 000 points, B = 16 (2-D, L1, squared, area: compute_winding_gpts' form), slices 1, 4 and automatic

and beside each the forward dn_winding_field at the same shape and, where it fits in memory (not at 128^3), float32 autograd of
winding_field_composed on the same GPU: its forward + backward against the fused forward + VJP, and its backward alone (the difference
of two timed arms) against the VJP.

Every arm is warmed up, then the arms are timed in rounds, one launch of each arm per round; the figure is the median over the rounds
with the smallest and largest value as the spread (as tools/bench_winding.py).

    python tools/bench_winding_vjp.py [--rounds 15] [--out profiles/winding_vjp.txt]
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_winding import fibonacci_sphere, time_arms  # noqa: E402
from diffnet_amd import _lib  # noqa: E402
from diffnet_amd.ops import winding_field, winding_field_vjp  # noqa: E402
from diffnet_amd.winding import winding_field_composed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winding_vjp.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def med(t):
        return t[len(t) // 2]

    def case(title, pts, nrm, area, q, metric, power, sweep, composed):
        B, npts, _ = pts.shape
        nq = q[0].numel()
        pairs = B * npts * nq
        g = (2.0 * torch.rand((B, nq), generator=torch.Generator().manual_seed(1)) - 1.0).to(dev)
        auto = _lib.lib().dn_winding_field_vjp_slices(B, npts, nq)
        arms = {"forward dn_winding_field": lambda: winding_field(pts, nrm, area, q, metric, power, 1.0)}
        for s in sweep + (0,):
            arms[f"vjp slices={s}" + (f" (automatic: {auto})" if s == 0 else "")] = lambda s=s: winding_field_vjp(pts, nrm, area, q, g, metric, power, 1.0, slices=s)
        if composed:
            leaves = [pts.clone().requires_grad_(True), nrm.clone().requires_grad_(True), area.clone().requires_grad_(True)]

            def comp_fwd():
                with torch.no_grad():
                    return winding_field_composed(pts, nrm, area, q, metric, power, 1.0)

            def comp_both():
                w = winding_field_composed(leaves[0], leaves[1], leaves[2], q, metric, power, 1.0)
                return torch.autograd.grad((w * g).sum(), leaves)

            arms["composed forward (no graph)"] = comp_fwd
            arms["composed forward + backward"] = comp_both
        t = time_arms(arms, a.rounds)
        say(f"--- {title}: B = {B}, {npts} points, {nq} queries, {pairs / 1e9:.3f} G pairs; automatic slices {auto}")
        for k, v in t.items():
            say(f"{k:38s} {med(v):11.1f} us (min {v[0]:.1f}, max {v[-1]:.1f}; {len(v)} rounds)  {pairs / med(v) / 1e3:8.1f} G pairs/s")
        f, v0 = med(t["forward dn_winding_field"]), med(next(v for k, v in t.items() if k.startswith("vjp slices=0")))
        say(f"vjp (automatic) / forward, time: {v0 / f:.2f} x")
        if composed:
            cb, cf = med(t["composed forward + backward"]), med(t["composed forward (no graph)"])
            say(f"composed forward + backward / fused forward + vjp: {cb / (f + v0):.1f} x;  composed backward alone (difference) / vjp: {(cb - cf) / v0:.1f} x")
            # the two routes agree (float32, other summation orders): largest difference relative to the largest gradient
            got = winding_field_vjp(pts, nrm, area, q, g, metric, power, 1.0)
            ref = comp_both()
            say("largest |fused - composed| / max |composed|: " + ", ".join(f"{n} {float((x - y).abs().max() / y.abs().max()):.1e}" for n, x, y in zip(("points", "normals", "area"), got, ref)))

    np3 = 10242
    unit = fibonacci_sphere(np3)
    m3 = unit[None].to(dev).contiguous()
    a3 = torch.full((1, np3), 4.0 * math.pi * 0.09 / np3, device=dev)
    q0 = torch.linspace(-0.5, 0.5, 25)
    qp = torch.stack(torch.meshgrid(q0, q0, q0, indexing="ij")).reshape(3, -1).to(dev).contiguous()
    case("probes 25^3", (0.3 * unit)[None].to(dev).contiguous(), m3, a3, qp, "l1", 3, (1, 4, 16, 64), True)
    x = torch.linspace(0.0, 1.0, 128)
    zz, yy, xx = torch.meshgrid(x, x, x, indexing="ij")
    q3 = torch.stack((xx, yy, zz)).reshape(3, -1).to(dev).contiguous()
    case("mesh 128^3", (0.5 + 0.3 * unit)[None].to(dev).contiguous(), m3, a3, q3, "l1", 3, (64, 256, 1024), False)
    B, npts, n = 16, 1000, 64
    th = torch.sort(torch.rand((B, npts), generator=torch.Generator().manual_seed(0)) * 2 * math.pi, dim=1).values
    p2 = torch.stack([0.5 + 0.3 * torch.cos(th), 0.5 + 0.3 * torch.sin(th)], -1).to(dev).contiguous()
    n2 = torch.stack([torch.cos(th), torch.sin(th)], -1).to(dev).contiguous()
    a2 = torch.full((B, npts), 2.0 * math.pi * 0.3 / npts, device=dev)
    x2 = torch.linspace(0.0, 1.0, n) + 0.5 / n                                  # nodes off the circle's own coordinates
    yy2, xx2 = torch.meshgrid(x2, x2, indexing="ij")
    q2 = torch.stack((xx2, yy2)).reshape(2, -1).to(dev).contiguous()
    case("2-D 64^2", p2, n2, a2, q2, "l1", 2, (1, 4), True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("tools/bench_winding_vjp.py: HIP-event times, median over rounds in which the arms alternate (spread: min, max)\n")
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
