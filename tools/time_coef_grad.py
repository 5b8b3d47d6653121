#!/usr/bin/env python3
"""Timings of the coefficient gradient of the Poisson losses (dn_poisson_coef_grad), event and host time, for profiles/coef_grad.txt.

  1. energy_loss(u, nu, f).backward() with all three requiring gradients, fused route against composed route (the switch
     dn_config_set("COEF_GRAD", "composed")), alternating in ONE process: 64^2 B=1 and 512^2 B=16.
  2. 2049^2 B=8: the bare coefficient launch (v absent: 12 B/node algorithmic, with v: 16 B/node) next to the transport forward on the
     same mesh.
  3. 128^3: the plain 3-D form next to the Poisson kernel (energy_loss_and_grad) on the same fields.

Every timed call works on one of `--sets` copies of its fields in rotation, so that the 256 MB last-level cache does not hold them from one
call to the next; a size is timed in `--rounds` rounds of `--reps` calls and the median round is reported.

    python tools/time_coef_grad.py [--reps 20] [--rounds 5] [--skip-3d]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd import DiffNet2DFEM, DiffNet3DFEM, _lib, ops  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, nsets, reps, rounds):
    """median over rounds of (device us per call by events, host us per call)"""
    for k in range(max(3, nsets)):
        fn(k % nsets)
    torch.cuda.synchronize()
    dev_us, host_us = [], []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for k in range(reps):
            fn(k % nsets)
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        dev_us.append(e0.elapsed_time(e1) * 1e3 / reps)
        host_us.append((t1 - t0) * 1e6 / reps)
    return statistics.median(dev_us), statistics.median(host_us)


def fields(shape, nsets, seed, lo=0.0):
    g = torch.Generator().manual_seed(seed)
    return [(lo + torch.rand(shape, generator=g)).to(DEV) for _ in range(nsets)]


def nsets_for(shape, nfields):
    nbytes = 4 * nfields
    for s in shape:
        nbytes *= s
    return max(2, min(8, int(600e6 // nbytes) + 1))


def backward_routes(n, B, a):
    m = DiffNet2DFEM(None, domain_size=n).to(DEV)
    shape = (B, 1, n, n)
    ns = nsets_for(shape, 6)
    us, nus, fs = fields(shape, ns, 1, -0.5), fields(shape, ns, 2, 0.5), fields(shape, ns, 3, -0.5)
    for t in us + nus + fs:
        t.requires_grad_(True)
    mask = torch.zeros((1, 1, n, n), device=DEV)
    mask[..., 0, :] = 1
    mask[..., :, 0] = 1

    def step(k):
        for t in (us[k], nus[k], fs[k]):
            t.grad = None
        m.energy_loss(us[k], nus[k], fs[k], dirichlet=[(mask, 0.0)], c=0.5).backward()

    res = {}
    for rnd in range(2):                     # alternate the routes: both see the same clocks
        for mode in ("fused", "composed"):
            _lib.config_set("COEF_GRAD", "composed" if mode == "composed" else "")
            res.setdefault(mode, []).append(timed(step, ns, a.reps, a.rounds))
    _lib.config_set("COEF_GRAD", "")
    out = {k: (min(d for d, _ in v), min(h for _, h in v)) for k, v in res.items()}
    print(f"energy_loss(u, nu, f).backward()  {n}^2 B={B}  sets={ns}")
    for mode in ("fused", "composed"):
        print(f"    {mode:9s} device {out[mode][0]:9.1f} us   host {out[mode][1]:9.1f} us")
    print(f"    ratio composed / fused: device {out['composed'][0] / out['fused'][0]:.2f}  host {out['composed'][1] / out['fused'][1]:.2f}")


def bare_2d(n, B, a):
    from diffnet_amd.transport import transport_residual
    m = DiffNet2DFEM(None, domain_size=n).to(DEV)
    shape = (B, 1, n, n)
    ns = nsets_for(shape, 4)
    us, vs = fields(shape, ns, 1, -0.5), fields(shape, ns, 2, -0.5)
    nodes = B * n * n
    print(f"bare launches  {n}^2 B={B}  sets={ns}")
    for name, fn, bpn in (("coef_grad v absent (nu, f)", lambda k: ops.poisson_coef_grad(m.geom, us[k], None, (), 1.0, -1.0, 1.0), 12),
                          ("coef_grad with v   (nu, f)", lambda k: ops.poisson_coef_grad(m.geom, us[k], vs[k], (), 1.0, -1.0, 1.0), 16),
                          ("coef_grad v absent (nu)", lambda k: ops.poisson_coef_grad(m.geom, us[k], None, (), 1.0, -1.0, 1.0, want="nu"), 8),
                          ("transport forward", lambda k: transport_residual(m, us[k], adv=(1.0, 0.5), kappa=(0.01, 0.01), tau=0.01), 8)):
        d, h = timed(fn, ns, a.reps, a.rounds)
        tbs = nodes * bpn / d / 1e6
        print(f"    {name:28s} device {d:8.1f} us  host {h:7.1f} us   {bpn:2d} B/node -> {tbs:5.2f} TB/s = {100 * tbs / 8.0:4.1f} % of 8 TB/s")


def plain_3d(n, a):
    m = DiffNet3DFEM(None, nsd=3, domain_size=n).to(DEV)
    shape = (1, 1, n, n, n)
    ns = nsets_for(shape, 4)
    us, nus, fs = fields(shape, ns, 1, -0.5), fields(shape, ns, 2, 0.5), fields(shape, ns, 3, -0.5)
    print(f"3-D plain form  {n}^3 B=1  sets={ns}")
    for name, fn in (("coef_grad v absent (nu, f)", lambda k: ops.poisson_coef_grad(m.geom, us[k], None, (), 1.0, -1.0, 1.0)),
                     ("coef_grad with v   (nu, f)", lambda k: ops.poisson_coef_grad(m.geom, us[k], fs[k], (), 1.0, -1.0, 1.0)),
                     ("energy_loss_and_grad (Poisson kernel)", lambda k: m.energy_loss_and_grad(us[k], nus[k], fs[k]))):
        d, h = timed(fn, ns, a.reps, a.rounds)
        print(f"    {name:38s} device {d:9.1f} us  host {h:7.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-3d", action="store_true")
    a = ap.parse_args()
    print(_lib.lib().dn_build_info().decode(), "|", torch.cuda.get_device_name(0))
    backward_routes(64, 1, a)
    backward_routes(512, 16, a)
    bare_2d(2049, 8, a)
    if not a.skip_3d:
        plain_3d(128, a)


if __name__ == "__main__":
    main()
