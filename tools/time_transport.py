#!/usr/bin/env python3
"""Times of the fused 2-D scalar transport operator (dn_transport_apply), after tools/time_ns.py: per mesh the forward and the VJP launch
of the linear (e17) and the reaction (e18) instantiation at 2, 3 and 4 Gauss points per axis next to the dn_ns_apply and dn_stokes_apply
forward on the same mesh in the same process, and at the scripts' size the loss + gradient by `transport_loss_and_grad` (two launches),
by autograd of `transport_loss` and by the composed route.  Every route runs on several buffer sets in rotation (nothing is served from
the last-level cache by the previous repetition), routes alternate in rounds, event time (device) and wall time (host) per call.

    python tools/time_transport.py [--reps 20] [--rounds 3] [--sizes 64:1,513:16,2049:8] [--ngp 2,3,4] [--no-composed]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd import DiffNet2DFEM, ops  # noqa: E402
from diffnet_amd.transport import transport_loss, transport_loss_and_grad, transport_residual_composed  # noqa: E402

E17 = dict(adv=(0.8660254, 0.5), kappa=(0.01, 0.01), tau=0.02, react=(0.0, 0.0, 0.0, 0.0))
E18 = dict(adv=(0.0, 1.0), kappa=(0.01, 0.01), tau=0.0, react=(-2.0, 32.0, -96.0, 64.0))


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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="64:1,513:16,2049:8")
    ap.add_argument("--ngp", default="2,3,4")
    ap.add_argument("--no-composed", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for spec in a.sizes.split(","):
        n, B = (int(x) for x in spec.split(":"))
        shape = (B, 1, n, n)
        nsets = max(2, min(8, int(1.5e9 // (4 * B * n * n * 8))))           # >= 2 sets, as many as fit next to the outputs
        wall = torch.zeros((1, 1, n, n), device=dev)
        wall[..., 0, :] = wall[..., -1, :] = wall[..., :, 0] = wall[..., :, -1] = 1.0
        wall = wall.to(torch.uint8)
        sets = [tuple(torch.rand(shape, device=dev) - 0.5 for _ in range(3)) for _ in range(nsets)]
        for ngp in (int(x) for x in a.ngp.split(",")):
            m = DiffNet2DFEM(None, domain_size=n, ngp_1d=ngp).to(dev)
            J = (0.5 * m.hx) * (0.5 * m.hy)
            routes = {}
            for tag, coef in (("e17", E17), ("e18", E18)):
                kw = dict(bc=(wall, None), bc_values=(1.0, 0.0), f_gp=0.3, wscale=J, **coef)
                routes[f"transport {tag} fwd"] = lambda s, kw=kw: ops.transport_apply(m.geom, s[0], None, **kw)
                routes[f"transport {tag} vjp"] = lambda s, kw=kw: ops.transport_apply(m.geom, s[0], None, cot=s[1], want_sums=False, **kw)
                routes[f"transport {tag} loss_and_grad"] = lambda s, kw=kw: transport_loss_and_grad(m, s[0], **kw)
                if n <= 128:
                    def auto(s, kw=kw):
                        u = s[0].detach().requires_grad_(True)
                        transport_loss(m, u, **kw).backward()
                    routes[f"transport {tag} loss + backward (autograd)"] = auto
                    if not a.no_composed:
                        def comp(s, kw=kw):
                            u = s[0].detach().requires_grad_(True)
                            (transport_residual_composed(m, u, **kw) ** 2).sum().backward()
                        routes[f"transport {tag} composed loss + backward"] = comp
            routes["ns fwd"] = lambda s: ops.ns_apply(m.geom, *s, wall, (1.0, 0.0, 0.0), 0.01, (0.3, 0.0), J, want_norms=True)
            routes["stokes fwd"] = lambda s: ops.stokes_apply(m.geom, *s, wall, (1.0, 0.0, 0.0), 0.01, 0.001, (0.3, 0.0), J, want_norms=True)
            best = {}
            for _ in range(a.rounds):
                for name, fn in routes.items():
                    ev, host = timed(fn, sets, a.reps)
                    if name not in best or ev < best[name][0]:
                        best[name] = (ev, host)
            nodes = B * n * n
            for name, (ev, host) in best.items():
                line = f"n {n} B {B} ngp {ngp}  {name:48s} event {ev:9.2f} us  host {host:9.2f} us"
                if name.startswith("transport") and name.endswith(("fwd", "vjp")):
                    nbytes = 8 * nodes + (4 * nodes if name.endswith("vjp") and "e18" in name else 0)
                    line += f"  {nbytes / ev / 1e6:6.3f} TB/s ({nbytes / ev / 1e6 / 8.0:5.3f} of 8 TB/s)"
                print(line, flush=True)


if __name__ == "__main__":
    main()
