#!/usr/bin/env python3
"""Times of the fused 2-D first-order-system least-squares loss (dn_fosls_apply), after tools/time_strongform.py: at the reference
script's own shape -- one packed (B, 3, 512, 512) parameter on Q1 with 2 Gauss points per axis, nodal nu and forcing, the wall fixed
through condition 2 -- at B = 1 and 16, and at 513^2 nodes Q2 with 3 Gauss points per axis at B = 1: the fused loss + gradient
(`fosls_loss_and_grad`, one launch), the same through autograd (`fosls_loss` + backward) and the composed route (`fosls_loss_composed` +
backward: 11 gauss_pt_eval launches, elementwise passes, autograd -- the loss written with the single-launch operators).
Every route runs on buffer sets in rotation, enough of them that their total exceeds the last-level cache (nothing is served from it by
the previous repetition), after a warm-up pass over every set; routes alternate in rounds; event time (device stream, first to last
launch) and wall time (host) per call; the best round of each is printed, with the ratio composed / fused, the algorithmic bytes of a
launch (five fields read: u, mx, my, nu, f; three written; the byte mask read) and the fraction of the HBM peak they amount to.

    python tools/time_fosls.py [--reps 40] [--rounds 5] [--shapes 512:1:1,512:1:16,513:2:1] [--no-composed]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd import DiffNet2DFEM  # noqa: E402
from diffnet_amd.fosls import fosls_loss, fosls_loss_and_grad, fosls_loss_composed  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, MI355X (HBM3E)
LLC_BYTES = 256 << 20      # Infinity Cache


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
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="512:1:1,512:1:16,513:2:1", help="n:degree:B,...")
    ap.add_argument("--no-composed", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for n, deg, B in (tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")):
        m = DiffNet2DFEM(None, domain_size=n, fem_basis_deg=deg).to(dev)
        tag = f"{n}^2 Q{deg} ngp {m.ngp_1d} B {B}"
        wall = torch.zeros((1, 1, n, n), device=dev)
        wall[..., 0, :] = wall[..., -1, :] = wall[..., :, 0] = wall[..., :, -1] = 1.0
        wall = wall.to(torch.uint8)
        nbytes = B * n * n * (8 * 4 + 1)                                       # 5 fields read, 3 written, the byte mask
        nsets = max(8, min(96, -(-2 * LLC_BYTES // (B * n * n * 5 * 4))))
        sets = [(torch.rand((B, 3, n, n), device=dev) - 0.5, 0.5 + torch.rand((B, 1, n, n), device=dev), torch.rand((B, 1, n, n), device=dev) - 0.5)
                for _ in range(nsets)]

        def kw(s):
            return dict(nu=s[1], bc=(None, wall), bc_values=(1.0, 0.0), f=s[2])

        def fused(s):
            return fosls_loss_and_grad(m, s[0], **kw(s))

        def auto(s):
            p = s[0].detach().requires_grad_(True)
            fosls_loss(m, p, **kw(s)).backward()

        def comp(s):
            p = s[0].detach().requires_grad_(True)
            fosls_loss_composed(m, p, **kw(s)).backward()

        routes = {"fused loss_and_grad (one launch)": fused, "fused loss + backward (autograd)": auto}
        if not a.no_composed:
            routes["composed loss + backward"] = comp
        best = {}
        for _ in range(a.rounds):
            for name, fn in routes.items():
                ev, host = timed(fn, sets, max(a.reps, nsets))
                if name not in best or ev < best[name][0]:
                    best[name] = (ev, host)
        for name, (ev, host) in best.items():
            print(f"{tag}  {name:36s} event {ev:9.2f} us  host {host:9.2f} us", flush=True)
        fe = best["fused loss_and_grad (one launch)"][0]
        print(f"{tag}  {nsets} buffer sets; algorithmic bytes per launch {nbytes / 1e6:.2f} MB -> {nbytes / (fe * 1e-6) / 1e12:.3f} TB/s, "
              f"{100 * nbytes / (fe * 1e-6) / HBM_PEAK:.1f} % of the HBM peak ({HBM_PEAK / 1e12:.0f} TB/s)", flush=True)
        if not a.no_composed:
            ce = best["composed loss + backward"][0]
            print(f"{tag}  composed / fused (event) {ce / fe:.1f} x, composed / fused through autograd "
                  f"{ce / best['fused loss + backward (autograd)'][0]:.1f} x", flush=True)


if __name__ == "__main__":
    main()
