#!/usr/bin/env python3
"""Timing of the fused 2-D Navier-Stokes (VMS) residual (dn_ns_apply) against the same residuals composed from the drop-in operators.

Per size, after a warm-up, the routes run alternately (round-robin, `--reps` rounds) in one process, each rep timed two ways:
  device  HIP events around the rep (start / end recorded on the current stream; the elapsed time of the pair)
  host    time.perf_counter() from before the call to after a torch.cuda.synchronize() that ends the rep
Routes:
  fwd        ops.ns_apply: the three residuals + their norms, one launch
  total_bwd  ns_total_loss(...).backward(): forward + VJP launch under autograd
  lag        ns_loss_and_grad: the same two launches without autograd
  composed   ns_residuals_composed + torch.norm, sum, backward (the scripts' body on the drop-in operators)
Median and minimum over the reps are printed per (size, route), with the algorithmic bytes of the forward (12 B read + 12 B written per
node and sample) and of the VJP (24 B read + 12 B written), the shared masks and lid values once, and their rates.

    python tools/time_ns.py [--reps 30] [--sizes 64:1,513:16,2049:8] [--ngp 2] [--no-composed] [--routes fwd,lag]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd import DiffNet2DFEM, ops  # noqa: E402
from diffnet_amd.navier_stokes import ns_loss_and_grad, ns_residuals_composed, ns_total_loss  # noqa: E402


def setup(n, B, dev, ngp=2):
    m = DiffNet2DFEM(None, domain_size=n, ngp_1d=ngp).to(dev)
    g = torch.Generator().manual_seed(1)
    flds = [(torch.rand((B, 1, n, n), generator=g) - 0.5).to(dev) for _ in range(3)]
    walls = torch.zeros((1, 1, n, n), device=dev)
    walls[..., 0, :] = 1.0
    walls[..., -1, :] = 1.0
    walls[..., :, 0] = 1.0
    walls[..., :, -1] = 1.0
    pin = torch.zeros((1, 1, n, n), device=dev)
    pin[..., 0, 0] = 1.0
    u_bc = torch.zeros((1, 1, n, n), device=dev)
    u_bc[..., -1, :] = 1.0 - 16.0 * (torch.linspace(0, 1, n, device=dev) - 0.5) ** 4
    Re = 100.0
    kw = dict(bc_values=(u_bc, 0.0, 0.0), visco=1.0 / Re, f_gp=None, wscale=(0.5 * m.h) ** 2)
    return m, flds, (walls, walls, pin), kw


def routes(m, flds, bc, kw, composed):
    geom = m.geom
    req = [f.clone().requires_grad_(True) for f in flds]

    def fwd():
        ops.ns_apply(geom, *flds, bc, kw["bc_values"], kw["visco"], kw["f_gp"], kw["wscale"], want_sums=False, want_norms=True)

    def total_bwd():
        for f in req:
            f.grad = None
        ns_total_loss(m, *req, bc, **kw).backward()

    def lag():
        ns_loss_and_grad(m, *flds, bc, **kw)

    def comp():
        for f in req:
            f.grad = None
        Rs = ns_residuals_composed(m, *req, bc, **kw)
        (torch.norm(Rs[0]) + torch.norm(Rs[1]) + torch.norm(Rs[2])).backward()

    r = dict(fwd=fwd, total_bwd=total_bwd, lag=lag)
    if composed:
        r["composed"] = comp
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="64:1,513:16,2049:8")
    ap.add_argument("--no-composed", action="store_true")
    ap.add_argument("--ngp", type=int, default=2, help="Gauss points per axis (the scripts use 2)")
    ap.add_argument("--routes", default="", help="comma-separated subset of fwd,total_bwd,lag,composed (default: all)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"{'size':>6} {'B':>3} {'route':>10} {'dev med us':>11} {'dev min us':>11} {'host med us':>12} {'host min us':>12}  note", flush=True)
    for spec in a.sizes.split(","):
        n, B = (int(x) for x in spec.split(":"))
        m, flds, bc, kw = setup(n, B, dev, a.ngp)
        rs = routes(m, flds, bc, kw, not a.no_composed)
        if a.routes:
            rs = {k: v for k, v in rs.items() if k in a.routes.split(",")}
        for fn in rs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ev = {k: [] for k in rs}
        host = {k: [] for k in rs}
        for _ in range(a.reps):
            for k, fn in rs.items():            # the routes alternate within every round
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                host[k].append((time.perf_counter() - t0) * 1e6)
                ev[k].append(e0.elapsed_time(e1) * 1e3)
        shared = n * n * (4 + 4 + 4 + 4)                         # the shared masks and lid values, once
        fwd_bytes = B * n * n * 24 + shared                      # fields in / residuals out per sample
        vjp_bytes = B * n * n * 36 + shared                      # fields and cotangents in / gradients out per sample
        for k in rs:
            dmed, dmin = statistics.median(ev[k]), min(ev[k])
            note = ""
            if k == "fwd":
                note = f"algorithmic {fwd_bytes / 1e6:.1f} MB -> {fwd_bytes / dmed / 1e6:.2f} TB/s at the median"
            elif k == "lag":
                note = f"algorithmic {(fwd_bytes + vjp_bytes) / 1e6:.1f} MB (fwd + vjp) -> {(fwd_bytes + vjp_bytes) / dmed / 1e6:.2f} TB/s at the median"
            print(f"{n:>6} {B:>3} {k:>10} {dmed:>11.1f} {dmin:>11.1f} {statistics.median(host[k]):>12.1f} {min(host[k]):>12.1f}  {note}", flush=True)
        del m, flds, rs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
