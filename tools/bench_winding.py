#!/usr/bin/env python3
"""Device time of the winding-number kernels, HIP events, in G point-query pairs per second:

  baseline   dn_winding_nodes (csrc/winding.hip), 512^2 nodes x 1000 points x B = 16
  2-D        dn_winding_field in the same setting (L1, cubed, no area, (4 pi)^-3), every tile and the automatic one
  3-D        128^3 nodes x 10 242 points: compute_winding_torch's form (L1, cubed, area), field and mask-only, every tile; the true
             winding number (L2, cubed) at the automatic tile
  probes     25^3 probes x 10 242 points, the reference script's own size, every tile; and a broadcast torch evaluation of the same
             sum (chunked over the probes), for the speed-up figure only

Every arm is warmed up, then the arms are timed in rounds, one launch of each arm per round, so that drift of the clock hits all of them
alike; the figure is the median over the rounds with the smallest and largest value as the spread.  The cloud is a Fibonacci sphere
(the reference's model.xyzna has 10 242 points too; the time does not depend on where the points are).

The one condition: the 3-D L1 kernel at 128^3 reaches at least 0.7 of the pairs/s of dn_winding_nodes in the same run (13 against 10
VALU issue slots per pair is 0.77 with nothing else gained).  Exit status 1 if it does not.

    python tools/bench_winding.py [--rounds 15] [--out profiles/winding_field.txt]
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffnet_amd import _lib  # noqa: E402
from diffnet_amd.ops import WINDING_TILES, compute_winding_nodes, winding_field  # noqa: E402


def fibonacci_sphere(npts):
    k = torch.arange(npts, dtype=torch.float64) + 0.5
    z = 1.0 - 2.0 * k / npts
    phi = math.pi * (1.0 + math.sqrt(5.0)) * k
    r = torch.sqrt(1.0 - z * z)
    return torch.stack((r * torch.cos(phi), r * torch.sin(phi), z), 1).float()


def time_arms(arms, rounds, warmup=3):
    """arms: name -> callable.  name -> sorted list of microseconds, one per round; the arms alternate inside every round."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    evs = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)] for k in arms}
    for r in range(rounds):
        for k, fn in arms.items():
            a, b = evs[k][r]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return {k: sorted(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in evs.items()}


def torch_broadcast(pts, nrm, area, q, chunk=1024):
    """the sum of compute_winding_torch as one broadcast expression per chunk of probes; q (3, nq)"""
    out = []
    for q0 in range(0, q.shape[1], chunk):
        d = pts[:, None, :, :] - q[:, q0:q0 + chunk].T[None, :, None, :]
        out.append((area[:, None, :] * (d * nrm[:, None]).sum(-1) / d.abs().sum(-1) ** 3).sum(-1))
    return torch.cat(out, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winding_field.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def report(title, pairs, times, names=None):
        res = {}
        for k in names or times:
            t = times[k]
            med = t[len(t) // 2]
            res[k] = pairs / med / 1e3
            lines.append(f"{title:34s} {k:26s} {med:10.1f} us (min {t[0]:.1f}, max {t[-1]:.1f}; {len(t)} rounds)  {res[k]:8.1f} G pairs/s "
                         f"(min {pairs / t[-1] / 1e3:.1f}, max {pairs / t[0] / 1e3:.1f})")
            print(lines[-1], flush=True)
        return res

    # ---- 2-D: the baseline and the general operator in its setting
    B, npts, n = 16, 1000, 512
    g = torch.Generator().manual_seed(0)
    th = torch.sort(torch.rand((B, npts), generator=g) * 2 * math.pi, dim=1).values
    pts = torch.stack([0.5 + 0.3 * torch.cos(th), 0.5 + 0.3 * torch.sin(th)], -1).to(dev).contiguous()
    nrm = torch.stack([torch.cos(th), torch.sin(th)], -1).to(dev).contiguous()
    zero = torch.zeros(B, 1, npts, 1, device=dev)
    xx, yy = torch.meshgrid(torch.linspace(0, 1, n), torch.linspace(0, 1, n), indexing="xy")
    nodes = torch.stack((xx, yy), 0).to(dev).contiguous()
    k2 = (4.0 * math.pi) ** -3
    arms = {"dn_winding_nodes": lambda: compute_winding_nodes(pts.unsqueeze(1), nrm.unsqueeze(1), zero, nodes)}
    for tile in (0,) + WINDING_TILES:
        arms[f"dn_winding_field tile={tile}"] = lambda tile=tile: winding_field(pts, nrm, None, nodes, "l1", 3, k2, tile=tile)
    # the 3-D arms go into the same rounds, so that the condition compares two figures of one run
    n3, np3 = 128, 10242
    unit = fibonacci_sphere(np3)
    p3 = (0.5 + 0.3 * unit)[None].to(dev).contiguous()
    m3 = unit[None].to(dev).contiguous()
    a3 = torch.full((1, np3), 4.0 * math.pi * 0.09 / np3, device=dev)
    x = torch.linspace(0.0, 1.0, n3)
    zz, yy3, xx3 = torch.meshgrid(x, x, x, indexing="ij")
    q3 = torch.stack((xx3, yy3, zz)).to(dev).contiguous()
    for tile in (0,) + WINDING_TILES:
        arms[f"3-D L1 field tile={tile}"] = lambda tile=tile: winding_field(p3, m3, a3, q3, "l1", 3, 1.0, tile=tile)
    arms["3-D L1 mask only tile=0"] = lambda: winding_field(p3, m3, a3, q3, "l1", 3, 1.0, want_field=False, want_mask=True)
    arms["3-D L2 field tile=0"] = lambda: winding_field(p3, m3, a3, q3, "l2", 3, 1.0 / (4.0 * math.pi))
    arms["3-D L2 mask only tile=0"] = lambda: winding_field(p3, m3, a3, q3, "l2", 3, 1.0 / (4.0 * math.pi), want_field=False, want_mask=True)
    t = time_arms(arms, a.rounds)
    lines.append(f"automatic tile: 2-D {_lib.lib().dn_winding_field_tile(B, n * n)}, 128^3 {_lib.lib().dn_winding_field_tile(1, n3 ** 3)}, "
                 f"25^3 {_lib.lib().dn_winding_field_tile(1, 25 ** 3)}")
    r2 = report(f"2-D {n}^2 x {npts} pts x B={B}", B * n * n * npts, t, [k for k in t if k.startswith("dn_")])
    r3 = report(f"3-D {n3}^3 x {np3} pts x B=1", n3 ** 3 * np3, t, [k for k in t if k.startswith("3-D")])

    # ---- the reference script's own size
    nprobe = 25
    q0 = torch.linspace(-0.5, 0.5, nprobe)
    qx, qy, qz = torch.meshgrid(q0, q0, q0, indexing="ij")
    qp = torch.stack((qx, qy, qz)).reshape(3, -1).to(dev).contiguous()
    pc = (0.3 * unit)[None].to(dev).contiguous()
    arms = {f"dn_winding_field tile={tile}": (lambda tile=tile: winding_field(pc, m3, a3, qp, "l1", 3, 1.0, tile=tile)) for tile in (0,) + WINDING_TILES}
    arms["torch broadcast"] = lambda: torch_broadcast(pc, m3, a3, qp)
    rp = report(f"probes {nprobe}^3 x {np3} pts x B=1", nprobe ** 3 * np3, time_arms(arms, a.rounds))

    base, new2, new3 = r2["dn_winding_nodes"], r2["dn_winding_field tile=0"], r3["3-D L1 field tile=0"]
    ok = new3 >= 0.7 * base
    lines.append(f"2-D setting: dn_winding_field / dn_winding_nodes = {new2 / base:.3f} (reported, not required)")
    lines.append(f"condition: 3-D L1 at 128^3 / dn_winding_nodes = {new3 / base:.3f} (required >= 0.7): {'met' if ok else 'NOT met'}")
    lines.append(f"25^3 probes: dn_winding_field (automatic tile) / torch broadcast = {rp['dn_winding_field tile=0'] / rp['torch broadcast']:.1f} x")
    for ln in lines[-3:]:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("tools/bench_winding.py: HIP-event times, median over rounds in which the arms alternate (spread: min, max)\n")
        fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
