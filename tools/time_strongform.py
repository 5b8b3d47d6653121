#!/usr/bin/env python3
"""Times of the fused 2-D strong-form least-squares loss (dn_strongform_apply), after tools/time_transport.py: at the reference scripts'
own shapes -- 257^2 nodes Q2 with the Burgers coefficients, 256^2 nodes Q3 with the strong-form Poisson coefficients and nodal forcing --
and B = 1 and 8, the fused loss + gradient (`strong_form_loss_and_grad`, one launch), the same through autograd (`strong_form_loss` +
backward) and the composed route (`strong_form_loss_composed` + backward: 2-4 gauss_pt_eval launches, elementwise passes, autograd).
Every route runs on several buffer sets in rotation (nothing is served from the last-level cache by the previous repetition), routes
alternate in rounds, event time (device stream, first to last launch) and wall time (host) per call; the best round of each is printed,
with the ratio composed / fused.

    python tools/time_strongform.py [--reps 20] [--rounds 5] [--batches 1,8]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd import DiffNet2DFEM  # noqa: E402
from diffnet_amd.strongform import (burgers_coefficients, poisson_strong_coefficients, strong_form_loss, strong_form_loss_and_grad,  # noqa: E402
                                    strong_form_loss_composed)


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
    ap.add_argument("--batches", default="1,8")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for tag, n, deg, coef, forcing in (("burgers 257^2 Q2", 257, 2, burgers_coefficients(), False),
                                       ("poisson 256^2 Q3", 256, 3, poisson_strong_coefficients(), True)):
        m = DiffNet2DFEM(None, domain_size=n, fem_basis_deg=deg).to(dev)
        wall = torch.zeros((1, 1, n, n), device=dev)
        wall[..., 0, :] = wall[..., -1, :] = wall[..., :, 0] = wall[..., :, -1] = 1.0
        wall = wall.to(torch.uint8)
        f = (torch.rand((1, 1, n, n), device=dev) - 0.5) if forcing else None
        kw = dict(bc=(None, wall), bc_values=(0.0, 0.0), f=f, coef=coef)
        for B in (int(x) for x in a.batches.split(",")):
            sets = [(torch.rand((B, 1, n, n), device=dev) - 0.5,) for _ in range(8)]

            def fused(s):
                return strong_form_loss_and_grad(m, s[0], **kw)

            def auto(s):
                u = s[0].detach().requires_grad_(True)
                strong_form_loss(m, u, **kw).backward()

            def comp(s):
                u = s[0].detach().requires_grad_(True)
                strong_form_loss_composed(m, u, **kw).backward()

            routes = {"fused loss_and_grad (one launch)": fused, "fused loss + backward (autograd)": auto, "composed loss + backward": comp}
            best = {}
            for _ in range(a.rounds):
                for name, fn in routes.items():
                    ev, host = timed(fn, sets, a.reps)
                    if name not in best or ev < best[name][0]:
                        best[name] = (ev, host)
            for name, (ev, host) in best.items():
                print(f"{tag} ngp {m.ngp_1d} B {B}  {name:36s} event {ev:9.2f} us  host {host:9.2f} us", flush=True)
            print(f"{tag} ngp {m.ngp_1d} B {B}  composed / fused (event) {best['composed loss + backward'][0] / best['fused loss_and_grad (one launch)'][0]:.1f} x, "
                  f"composed / fused through autograd {best['composed loss + backward'][0] / best['fused loss + backward (autograd)'][0]:.1f} x", flush=True)


if __name__ == "__main__":
    main()
