#!/usr/bin/env python3
"""Times of the fused 2-D eikonal residual (dn_eikonal_apply), after tools/time_transport.py: per shape the forward launch (R and its
norm), the VJP launch and the pair `eikonal_loss_and_grad` (two launches) next to (a) the composed route + autograd
(`eikonal_residual_composed`, norm, backward) and (b) the `helmholtz_residual_loss_and_grad` pair, which runs on the same element march
(its forward moves the same bytes, its second launch reads one array less than the eikonal VJP), in the same process.  Every route runs
on several buffer sets in rotation (nothing is served from the last-level cache by the previous repetition), routes alternate in rounds,
event time (device) and wall time (host) per call; the best round of each is printed with the spread of the rounds, the algorithmic
bandwidth of the eikonal launches (fp32 arrays a launch must move: u, the uint8 mask as a quarter, R | u, cot, mask, grad) and both ratios.

    python tools/time_eikonal.py [--reps 20] [--rounds 5] [--shapes 1:2:512:16,2:3:1025:1] [--no-composed]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd import DiffNet2DFEM, ops  # noqa: E402
from diffnet_amd import eikonal as ek  # noqa: E402
from diffnet_amd import helmholtz as hh  # noqa: E402


def timed(fn, sets, reps):
    """(event us, wall us) per call of fn(set) over the sets in rotation"""
    for s in sets:
        fn(s)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(reps):
        fn(sets[i % len(sets)])
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, (t1 - t0) * 1e6 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="1:2:512:16,2:3:1025:1", help="degree:ngp:n:B")
    ap.add_argument("--no-composed", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for spec in a.shapes.split(","):
        P, ngp, n, B = (int(x) for x in spec.split(":"))
        shape = (B, 1, n, n)
        nbytes = 4 * B * n * n
        nsets = max(2, min(96, -(-2 * (256 << 20) // nbytes)))            # the fields u of one rotation exceed twice the last-level cache
        m = DiffNet2DFEM(None, domain_size=n, fem_basis_deg=P, ngp_1d=ngp).to(dev)
        wall = torch.zeros((1, 1, n, n), device=dev)
        wall[..., 0, :] = wall[..., -1, :] = wall[..., :, 0] = wall[..., :, -1] = 1.0
        wall = wall.to(torch.uint8)
        x = torch.linspace(0.0, 1.0, n, device=dev)
        dist = torch.hypot(x[None, :] - 0.5, x[:, None] - 0.5) - 0.3
        sets = [(dist + m.hx * (torch.rand(shape, device=dev) - 0.5), torch.rand(shape, device=dev) - 0.5) for _ in range(nsets)]
        kw = dict(bc=(wall, None), bc_values=(0.0, 0.0), tau=0.25)
        J = (0.5 * m.hx) * (0.5 * m.hy)
        hkw = dict(sigma=9.0, bc=(wall, None), bc_values=(0.0, 0.0), f_gp=1.0, wscale=J)

        def comp(s):
            u = s[0].detach().requires_grad_(True)
            torch.norm(ek.eikonal_residual_composed(m, u, **kw)).backward()

        routes = {
            "eikonal fwd (R + norm)": lambda s: ops.eikonal_apply(m.geom, s[0], kw["bc"], kw["bc_values"], tau=0.25, wscale=J, want_norm=True),
            "eikonal vjp": lambda s: ops.eikonal_apply(m.geom, s[0], kw["bc"], kw["bc_values"], tau=0.25, wscale=J, cot=s[1]),
            "eikonal loss_and_grad (two launches)": lambda s: ek.eikonal_loss_and_grad(m, s[0], **kw),
            "helmholtz residual_loss_and_grad (two launches)": lambda s: hh.helmholtz_residual_loss_and_grad(m, s[0], **hkw),
        }
        if not a.no_composed:
            routes["eikonal composed norm + backward"] = comp
        best, worst = {}, {}
        for _ in range(a.rounds):
            for name, fn in routes.items():
                ev, host = timed(fn, sets, max(a.reps, nsets))
                if name not in best or ev < best[name][0]:
                    best[name] = (ev, host)
                worst[name] = max(worst.get(name, 0.0), ev)
        tag = f"Q{P} ngp {ngp} {n}^2 B {B} ({nsets} sets)"
        arrays = {"eikonal fwd (R + norm)": 2.25, "eikonal vjp": 3.25, "eikonal loss_and_grad (two launches)": 5.5}
        for name, (ev, host) in best.items():
            line = f"{tag}  {name:48s} event {ev:9.2f} us (worst round {worst[name]:9.2f})  host {host:9.2f} us"
            if name in arrays:
                line += f"  {arrays[name] * nbytes / ev / 1e6:6.3f} TB/s"
            print(line, flush=True)
        pair = best["eikonal loss_and_grad (two launches)"][0]
        line = f"{tag}  eikonal pair / helmholtz pair (event): {pair / best['helmholtz residual_loss_and_grad (two launches)'][0]:.3f}"
        if not a.no_composed:
            line += f"; composed / fused: {best['eikonal composed norm + backward'][0] / pair:.1f} x"
        print(line, flush=True)


if __name__ == "__main__":
    main()
