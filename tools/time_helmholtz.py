#!/usr/bin/env python3
"""Times of the fused 2-D Helmholtz energy and residual losses (dn_helmholtz_apply), after tools/time_strongform.py: at the reference
scripts' own shape -- 64^2 nodes Q1, B = 1, the RectangleHelmholtzManufactured sample -- and at 512^2 nodes Q1 with B = 16, the fused
energy + gradient (`helmholtz_energy_loss_and_grad`, one launch), the same through autograd (`helmholtz_energy_loss` + backward), the
composed route (`helmholtz_energy_loss_composed` + backward: 5 gauss_pt_eval launches, elementwise passes, autograd) and the residual
loss + gradient, fused (two launches) and composed.  Every route runs on buffer sets in rotation: enough of them that the fields u of
one rotation exceed twice the 256 MiB last-level cache (at most 96 sets: the 64^2 shape stays cache resident, as it is in a training
loop), routes alternate in rounds, event time (device stream, first to last launch) and wall time (host) per call; the best round of each
is printed, with the number of sets and the ratio composed / fused.

    python tools/time_helmholtz.py [--reps 20] [--rounds 5] [--shapes 64:1,512:16]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd import DiffNet2DFEM  # noqa: E402
from diffnet_amd import helmholtz as hh  # noqa: E402
from diffnet_amd.datasets.single_instances.rectangles import RectangleHelmholtzManufactured  # noqa: E402

LLC_BYTES = 256 << 20


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
    ap.add_argument("--shapes", default="64:1,512:16", help="n:B pairs")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for n, B in (tuple(int(x) for x in p.split(":")) for p in a.shapes.split(",")):
        ds = RectangleHelmholtzManufactured(domain_size=n)
        inputs, forcing = ds[0]
        inputs, forcing = inputs[None].to(dev), forcing[None].to(dev)
        m = DiffNet2DFEM(None, domain_size=n).to(dev)
        kw = dict(nu=inputs[:, 0:1].contiguous(), bc=(inputs[:, 1:2].contiguous(), inputs[:, 2:3].contiguous()), bc_values=(1.0, 0.0),
                  f=forcing.contiguous())
        coef = hh.helmholtz_coefficients(ds.khh)
        nsets = max(8, min(96, -(-2 * LLC_BYTES // (B * n * n * 4))))
        sets = [(torch.rand((B, 1, n, n), device=dev) - 0.5,) for _ in range(nsets)]

        def fused(s):
            return hh.helmholtz_energy_loss_and_grad(m, s[0], **kw, **coef)

        def auto(s):
            u = s[0].detach().requires_grad_(True)
            hh.helmholtz_energy_loss(m, u, **kw, **coef).backward()

        def comp(s):
            u = s[0].detach().requires_grad_(True)
            hh.helmholtz_energy_loss_composed(m, u, **kw, **coef).backward()

        def res_fused(s):
            return hh.helmholtz_residual_loss_and_grad(m, s[0], sigma=coef["sigma"], **kw)

        def res_comp(s):
            u = s[0].detach().requires_grad_(True)
            torch.sum(hh.helmholtz_residual_composed(m, u, sigma=coef["sigma"], **kw) ** 2).backward()

        routes = {"energy fused loss_and_grad (one launch)": fused, "energy fused loss + backward (autograd)": auto,
                  "energy composed loss + backward": comp, "residual fused loss_and_grad (two launches)": res_fused,
                  "residual composed loss + backward": res_comp}
        best = {}
        for _ in range(a.rounds):
            for name, fn in routes.items():
                ev, host = timed(fn, sets, max(a.reps, nsets))
                if name not in best or ev < best[name][0]:
                    best[name] = (ev, host)
        tag = f"helmholtz mms {n}^2 Q1 ngp {m.ngp_1d} B {B} ({nsets} buffer sets)"
        for name, (ev, host) in best.items():
            print(f"{tag}  {name:44s} event {ev:9.2f} us  host {host:9.2f} us", flush=True)
        print(f"{tag}  composed / fused (event): energy {best['energy composed loss + backward'][0] / best['energy fused loss_and_grad (one launch)'][0]:.1f} x, "
              f"residual {best['residual composed loss + backward'][0] / best['residual fused loss_and_grad (two launches)'][0]:.1f} x", flush=True)


if __name__ == "__main__":
    main()
