#!/usr/bin/env python3
"""Times of the fused 3-D eikonal residual (dn_eikonal3d_apply), after tools/time_eikonal.py: per shape the forward launch (R and its
norm), the VJP launch and the pair `eikonal_loss_and_grad` (two launches) next to (a) the composed route + autograd
(`eikonal_residual_composed`, norm, backward), which uses only the drop-in operators, and (b) the 3-D Q1 Poisson `residual_loss` launch on
the same mesh, which moves the same class of bytes (one field in, one out), in the same process.  Every route runs on several buffer
sets in rotation (nothing is served from the last-level cache by the previous repetition), routes alternate in rounds, event time
(device) and wall time (host) per call; the best round of each is printed with the spread of the rounds, the algorithmic bandwidth of
the eikonal launches (fp32 arrays a launch must move: u, the uint8 mask as a quarter, R | u, cot, mask, grad) as a fraction of the
HBM peak (8 TB/s) and both ratios.  The composed route is heavy (tens of GB of intermediates at 256^3): it runs fewer repetitions and
a shape on which it runs out of memory is reported as such.

    python tools/time_eikonal3d.py [--reps 20] [--rounds 3] [--shapes 2:64:8,2:128:1,...] [--no-composed] [--masks 0,1]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd import DiffNet3DFEM, ops  # noqa: E402
from diffnet_amd import eikonal as ek  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s (MI355X, specification)


def timed(fn, sets, reps):
    """(event us, wall us) per call of fn(set) over the sets in rotation"""
    for s in sets[:max(1, min(len(sets), reps))]:
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--composed-reps", type=int, default=3)
    ap.add_argument("--shapes", default="2:64:8,3:64:8,2:128:1,3:128:1,2:128:4,3:128:4,2:256:1,3:256:1", help="ngp:n:B")
    ap.add_argument("--masks", default="0,1", help="0: no condition, 1: a uint8 wall mask")
    ap.add_argument("--no-composed", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for spec in a.shapes.split(","):
        ngp, n, B = (int(x) for x in spec.split(":"))
        shape = (B, 1, n, n, n)
        nbytes = 4 * B * n ** 3
        nsets = max(2, min(96, -(-2 * (256 << 20) // nbytes)))            # the fields u of one rotation exceed twice the last-level cache
        m = DiffNet3DFEM(None, domain_size=n, nsd=3, ngp_1d=ngp).to(dev)
        wall = torch.zeros((1, 1, n, n, n), device=dev)
        wall[..., 0, :, :] = wall[..., -1, :, :] = wall[..., :, 0, :] = wall[..., :, -1, :] = wall[..., :, :, 0] = wall[..., :, :, -1] = 1.0
        wall = wall.to(torch.uint8)
        x = torch.linspace(0.0, 1.0, n, device=dev)
        dist = torch.sqrt((x[None, None, :] - 0.5) ** 2 + (x[None, :, None] - 0.5) ** 2 + (x[:, None, None] - 0.5) ** 2) - 0.3
        sets = [(dist + m.hx * (torch.rand(shape, device=dev) - 0.5), torch.rand(shape, device=dev) - 0.5) for _ in range(nsets)]
        J = (0.5 * m.hx) * (0.5 * m.hy) * (0.5 * m.hz)
        for masked in (int(x) for x in a.masks.split(",")):
            bc = (wall, None) if masked else None
            kw = dict(bc=bc, bc_values=(0.0, 0.0), tau=0.25)
            dl = [(wall, 0.0)] if masked else ()

            def comp(s):
                u = s[0].detach().requires_grad_(True)
                torch.norm(ek.eikonal_residual_composed(m, u, **kw)).backward()

            routes = {
                "eikonal3d fwd (R + norm)": lambda s: ops.eikonal3d_apply(m.geom, s[0], bc, (0.0, 0.0), tau=0.25, wscale=J, want_norm=True),
                "eikonal3d vjp": lambda s: ops.eikonal3d_apply(m.geom, s[0], bc, (0.0, 0.0), tau=0.25, wscale=J, cot=s[1]),
                "eikonal3d loss_and_grad (two launches)": lambda s: ek.eikonal_loss_and_grad(m, s[0], **kw),
                "poisson3d residual_loss (one launch)": lambda s: m.residual_loss(s[0], dirichlet=dl),
            }
            best, worst = {}, {}
            for _ in range(a.rounds):
                for name, fn in routes.items():
                    ev, host = timed(fn, sets, max(a.reps, nsets))
                    if name not in best or ev < best[name][0]:
                        best[name] = (ev, host)
                    worst[name] = max(worst.get(name, 0.0), ev)
            composed = None
            if not a.no_composed:
                try:
                    for _ in range(2):
                        ev, host = timed(comp, sets, a.composed_reps)
                        if composed is None or ev < composed[0]:
                            composed = (ev, host)
                        worst["composed"] = max(worst.get("composed", 0.0), ev)
                except torch.OutOfMemoryError:
                    composed = "out of memory"
                    torch.cuda.empty_cache()
            tag = f"Q1 ngp {ngp} {n}^3 B {B} mask {'u8' if masked else 'none'} ({nsets} sets)"
            mk = 0.25 if masked else 0.0
            arrays = {"eikonal3d fwd (R + norm)": 2.0 + mk, "eikonal3d vjp": 3.0 + mk, "eikonal3d loss_and_grad (two launches)": 5.0 + 2 * mk,
                      "poisson3d residual_loss (one launch)": 2.0 + mk}
            for name, (ev, host) in best.items():
                bw = arrays[name] * nbytes / (ev * 1e-6)
                print(f"{tag}  {name:40s} event {ev:10.2f} us (worst round {worst[name]:10.2f})  host {host:10.2f} us  {bw / 1e12:6.3f} TB/s = "
                      f"{100 * bw / HBM_PEAK:5.1f} % of the HBM peak", flush=True)
            fwd, pair = best["eikonal3d fwd (R + norm)"][0], best["eikonal3d loss_and_grad (two launches)"][0]
            line = f"{tag}  eikonal3d fwd / poisson3d residual_loss (event): {fwd / best['poisson3d residual_loss (one launch)'][0]:.3f}"
            if isinstance(composed, tuple):
                print(f"{tag}  {'eikonal composed norm + backward':40s} event {composed[0]:10.2f} us (worst round {worst['composed']:10.2f})  host {composed[1]:10.2f} us",
                      flush=True)
                line += f"; composed / fused pair: {composed[0] / pair:.1f} x"
            elif composed is not None:
                line += f"; composed: {composed}"
            print(line, flush=True)
        del sets, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
