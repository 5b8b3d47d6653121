#!/usr/bin/env python3
"""Device time of the 3-D Q1 Poisson launches a change to their kernels is judged on, one line per row, "<row>: <us>":
the five 3-D Poisson rows of bench.py's config list (128^3 and 256^3, B = 1, the exact 2-point rule: uint8 mask image; load vector; load
vector + box faces + sums folded into the next launch) as prepared launches (ops.PoissonPlan) on four sets of arrays in rotation, one row per
remaining kernel family at 128^3, B = 1, nu, nodal f, one uint8 image (3d_q1_n2 under "Q1_3D_E1SUM", 3d_q1_n1 under "Q1_3D_E1", 3d_q1_t16
under "Q1_3D_T16", 3d_q1_generic at 3 and 4 points, 3d_q1_n1 at 3 points under "PLAN3D" = "16,16,1,8"; dn_poisson_query must name the family
before a row is timed), and eikonal3d_apply forward at 128^3.  The launches are enqueued behind a blocker kernel, so HIP events see no host gaps.
One process measures one library (DN_LIB_PATH); compare processes, alternating, for an A/B.

Usage: python tools/time_poisson3d_rows.py [--reps 60]
"""
import argparse
import ctypes as C
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd import BoxFaces, DiffNet3DFEM, LoadVector, _lib, ops  # noqa: E402

DEV = torch.device("cuda:0")
FAM = {4: "3d_q1_n1", 5: "3d_q1_t16", 6: "3d_q1_generic", 7: "3d_q1_n2", 8: "3d_q1_cfz"}
_CYC_PER_US = None


def timed(fn, n):
    global _CYC_PER_US
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if _CYC_PER_US is None:
        torch.cuda._sleep(1000); torch.cuda.synchronize()
        a.record(); torch.cuda._sleep(10_000_000); b.record(); torch.cuda.synchronize()
        _CYC_PER_US = 10_000_000 / (a.elapsed_time(b) * 1e3)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.04:          # 40 ms of load first: a GPU that has just left idle runs 10-25 % slower (tools/ramp2d.py)
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    host_us = (time.perf_counter() - t0) / n * 1e6
    torch.cuda.synchronize()
    torch.cuda._sleep(int(_CYC_PER_US * host_us * n * 3.0) + 1000)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    u, nu, f = (torch.rand(shape, generator=g).to(DEV) for _ in range(3))
    bc = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    for d in range(2, len(shape)):
        idx = [slice(None)] * len(shape); idx[d] = 0; bc[tuple(idx)] = 1; idx[d] = -1; bc[tuple(idx)] = 1
    return u, nu + 0.5, f, bc


def poisson_row(name, n, ngp, reps, family, c=0.5, load=False, box=False, fold=False, switches=()):
    for k, v in switches:
        _lib.config_set(k, v)
    ops.call_cache_clear()
    m = DiffNet3DFEM(None, domain_size=n, ngp_1d=ngp, nsd=3).to(DEV)
    shape = (1, 1, *m.geom.node_shape)
    scale = 1.0 / m.geom.nelem_total
    plans = []
    for k in range(4):
        u, nu, f, bc = inputs(shape, 7 + k)
        if load:
            f = LoadVector.assemble(m.geom, f)
        plans.append(ops.PoissonPlan(m.geom, u, nu, f, None, [(BoxFaces("all"), 0.0)] if box else [(bc, 0.0)], alpha=2.0 * c, beta=1.0, c=c, wscale=1.0,
                                     out_scale=scale, want_out=True, want_sums=True, loss_scale=scale, out=torch.empty(shape, device=DEV), pipelined_sums=fold))
    if fold:
        for k in range(4):
            plans[k].fold(plans[k - 1])
    q = _lib.DnPoissonKernel()
    rc = _lib.lib().dn_poisson_query(C.byref(plans[0].mesh), C.byref(plans[0].args), C.byref(q))
    if rc != 0 or FAM.get(q.family) != family:
        raise SystemExit(f"{name}: dn_poisson_query gives {rc}, {FAM.get(q.family)}; the row is meant for {family}")
    turn = [0]

    def fn():
        turn[0] = (turn[0] + 1) % 4
        plans[turn[0]].launch()

    us = timed(fn, reps)
    print(f"{name} [{family}]: {us:.2f}", flush=True)
    for k, _ in switches:
        _lib.config_set(k, "")


def eikonal_row(reps):
    m = DiffNet3DFEM(None, domain_size=128, ngp_1d=2, nsd=3).to(DEV)
    shape = (1, 1, *m.geom.node_shape)
    sets = [inputs(shape, 40 + k) for k in range(4)]
    turn = [0]

    def fn():
        turn[0] = (turn[0] + 1) % 4
        u, _, _, bc = sets[turn[0]]
        ops.eikonal3d_apply(m.geom, u, (bc, None), (0.0, 0.0), tau=0.05, want_norm=True)

    print(f"eikonal3d 128^3 B=1 forward: {timed(fn, reps):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    r = ap.parse_args().reps
    poisson_row("cfg3 128^3", 128, 2, r, "3d_q1_cfz")
    poisson_row("cfg3 128^3 load vector + box faces + folded sums", 128, 2, r, "3d_q1_cfz", load=True, box=True, fold=True)
    poisson_row("cfg4 256^3", 256, 2, r, "3d_q1_cfz", c=1.0)
    poisson_row("cfg4 256^3 load vector", 256, 2, r, "3d_q1_cfz", c=1.0, load=True)
    poisson_row("cfg4 256^3 load vector + box faces + folded sums", 256, 2, r, "3d_q1_cfz", c=1.0, load=True, box=True, fold=True)
    poisson_row("128^3 Q1_3D_E1SUM", 128, 2, r, "3d_q1_n2", switches=[("Q1_3D_E1SUM", "1")])
    poisson_row("128^3 Q1_3D_E1", 128, 2, r, "3d_q1_n1", switches=[("Q1_3D_E1", "1")])
    poisson_row("128^3 Q1_3D_T16", 128, 2, r, "3d_q1_t16", switches=[("Q1_3D_T16", "1")])
    poisson_row("128^3 3 points", 128, 3, r, "3d_q1_generic")
    poisson_row("128^3 3 points PLAN3D=16,16,1,8", 128, 3, r, "3d_q1_n1", switches=[("PLAN3D", "16,16,1,8")])
    poisson_row("128^3 4 points", 128, 4, r, "3d_q1_generic")
    eikonal_row(r)
    return 0


if __name__ == "__main__":
    sys.exit(main())
