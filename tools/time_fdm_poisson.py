#!/usr/bin/env python3
"""Times of the fused 2-D finite-difference Poisson residual loss (dn_fdm_poisson_apply), after tools/time_eikonal3d.py: per shape the
fused forward (the sums alone: the loss without its gradient), the fused loss + gradient -- one launch for the mean of squares, two
for the per-sample L2 norm -- next to the composed twin's loss + backward (`DiffNetFDM.composed_poisson_residual_loss`: torch.where,
six conv2d calls, the elementwise passes, autograd: the route as it stands without the fused operator) and to dn_probe_stream over the
same four arrays (u, nu, f read, the gradient written: the floor a streaming kernel reaches), in the same process.  Every route runs
on several buffer sets in rotation (nothing is served from the last-level cache by the previous repetition), routes alternate in
rounds, event time (device) and wall time (host) per call; the best round of each is printed with the spread of the rounds, the
algorithmic bandwidth of the fused launches (the fp32 arrays a launch must move: u, nu, f, the gradient, the masks where present) as
a fraction of the HBM peak (8 TB/s) and the ratios composed / fused and fused / stream floor.

    python tools/time_fdm_poisson.py [--reps 20] [--rounds 3] [--shapes 64:1,256:16,512:64,513:63] [--masks 0,2]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd import _lib, ops  # noqa: E402
from diffnet_amd.fdm import DiffNetFDM  # noqa: E402

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
    ap.add_argument("--shapes", default="64:1,256:16,512:64,513:63", help="n:B")
    ap.add_argument("--masks", default="0,2", help="0: no condition, 2: the two fp32 per-sample masks of the scripts' datasets")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    for spec in a.shapes.split(","):
        n, B = (int(x) for x in spec.split(":"))
        shape = (B, 1, n, n)
        nbytes = 4 * B * n * n
        nsets = max(2, min(96, -(-2 * (256 << 20) // nbytes)))            # the fields u of one rotation exceed twice the last-level cache
        m = DiffNetFDM(None, domain_size=n).to(dev)
        bc1, bc2 = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
        bc1[..., :, 0] = 1.0
        bc2[..., :, -1] = 1.0
        sets = [(torch.rand(shape, device=dev), 0.5 + torch.rand(shape, device=dev), torch.rand(shape, device=dev) - 0.5) for _ in range(nsets)]
        out = torch.empty(shape, device=dev)
        nstream = (B * n * n) // 4 * 4
        for masked in (int(x) for x in a.masks.split(",")):
            bc = (bc1, bc2) if masked else ()
            kw = dict(bc=bc, bc_values=(1.0, 0.0))

            def comp(norm):
                def run(s):
                    u = s[0].detach().requires_grad_(True)
                    m.composed_poisson_residual_loss(u, s[1], s[2], norm=norm, **kw).backward()
                return run

            def stream(s):
                lib.dn_probe_stream(s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), out.data_ptr(), nstream, 0, ops._stream(out))

            routes = {
                "fused forward (sums alone)": lambda s: ops.fdm_poisson_apply(s[0], s[1], s[2], bc=bc or None, bc_values=(1.0, 0.0), want_grad=False),
                "fused mean_sq loss + grad (one launch)": lambda s: m.poisson_residual_loss_and_grad(s[0], s[1], s[2], norm="mean_sq", **kw),
                "fused l2 loss + grad (two launches)": lambda s: m.poisson_residual_loss_and_grad(s[0], s[1], s[2], norm="l2", **kw),
                "composed mean_sq loss + backward": comp("mean_sq"),
                "composed l2 loss + backward": comp("l2"),
                "dn_probe_stream (3 read, 1 written)": stream,
            }
            best, worst = {}, {}
            for _ in range(a.rounds):
                for name, fn in routes.items():
                    ev, host = timed(fn, sets, max(a.reps, nsets))
                    if name not in best or ev < best[name][0]:
                        best[name] = (ev, host)
                    worst[name] = max(worst.get(name, 0.0), ev)
            tag = f"{n}^2 B {B} masks {'2 x fp32' if masked else 'none'} ({nsets} sets)"
            mk = float(masked)
            arrays = {"fused forward (sums alone)": 3.0 + mk, "fused mean_sq loss + grad (one launch)": 4.0 + mk,
                      "fused l2 loss + grad (two launches)": 7.0 + 2 * mk, "dn_probe_stream (3 read, 1 written)": 4.0}
            for name, (ev, host) in best.items():
                line = f"{tag}  {name:40s} event {ev:10.2f} us (worst round {worst[name]:10.2f})  host {host:10.2f} us"
                if name in arrays:
                    bw = arrays[name] * nbytes / (ev * 1e-6)
                    line += f"  {bw / 1e12:6.3f} TB/s = {100 * bw / HBM_PEAK:5.1f} % of the HBM peak"
                print(line, flush=True)
            one, two, floor = (best[k][0] for k in ("fused mean_sq loss + grad (one launch)", "fused l2 loss + grad (two launches)",
                                                    "dn_probe_stream (3 read, 1 written)"))
            print(f"{tag}  composed / fused: mean_sq {best['composed mean_sq loss + backward'][0] / one:.1f} x, l2 "
                  f"{best['composed l2 loss + backward'][0] / two:.1f} x; fused mean_sq pair / stream floor: {one / floor:.2f}", flush=True)
        del sets, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
