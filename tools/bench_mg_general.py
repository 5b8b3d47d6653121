#!/usr/bin/env python3
"""Measurements of multigrid on meshes that are not nested (mg_coarsening="general": dn_poisson_mg_transfer, diffnet_amd/solve.py;
profiles/poisson_multigrid_general.txt).  Needs an MI355X.

    python tools/bench_mg_general.py --transfers      # the general RESTRICT / PROLONG at 512^2 B = 16 and 256^3 beside the nested kernels at
                                                      # 513^2 B = 16 and 257^3: a launch captured `--iters` times in a HIP graph, replayed,
                                                      # device events, median; bytes = (2 n_fine + n_coarse) floats per sample
    python tools/bench_mg_general.py --convergence    # iterations and wall time of one poisson_solve to tol = 1e-5 (random nu in [0.5, 1.5],
                                                      # random f, u = 0 on the box faces): general multigrid against Jacobi at 2^k nodes per
                                                      # axis, the nested solve one node larger beside it, and the mms example at n = 128"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
from bench_solve import geometry, graph_median_us  # noqa: E402
from diffnet_amd import BoxFaces, ops, solve  # noqa: E402


def transfers(iters, replays):
    dev = torch.device("cuda")
    rows = {}
    for kind, shape, B in (("general", (512, 512), 16), ("nested", (513, 513), 16), ("general", (256, 256, 256), 1), ("nested", (257, 257, 257), 1)):
        cshape = ops.mg_general_coarse_shape(shape) if kind == "general" else tuple((s - 1) // 2 + 1 for s in shape)
        nf, nc = int(np.prod(shape)), int(np.prod(cshape))
        g = torch.Generator().manual_seed(2)
        b, q, x = (torch.randn((B, nf), generator=g).to(dev) for _ in range(3))
        c = torch.randn((B, nc), generator=g).to(dev)
        fm = (torch.rand((1, nf), generator=g) < 0.05).to(torch.uint8).to(dev)
        cm = (torch.rand((1, nc), generator=g) < 0.05).to(torch.uint8).to(dev)
        if kind == "general":
            tables = ops.MgTransferTables(shape, dev)
            ar, keep_r = ops.poisson_mg_transfer_args("restrict", shape, B, tables, b=b, q=q, c=c, mask=cm)
            ap, keep_p = ops.poisson_mg_transfer_args("prolong", shape, B, tables, x=x, c=c, mask=fm)
            launch = ops.poisson_mg_transfer_launch
        else:
            ar, keep_r = ops.poisson_mg_args("restrict", shape, B, b=b, q=q, c=c, mask=cm)
            ap, keep_p = ops.poisson_mg_args("prolong", shape, B, x=x, c=c, mask=fm)
            launch = ops.poisson_mg_launch
        mb = (2 * nf + nc) * 4.0 * B / 1e6
        for op, a in (("restrict", ar), ("prolong", ap)):
            us = graph_median_us(lambda: launch(a, dev), iters, replays)
            rows[(kind, len(shape), op)] = us[0]
            print(f"{kind:>8} {op:>8} {'x'.join(map(str, shape)):>12} -> {'x'.join(map(str, cshape)):>12} B={B:<2}: {us[0]:7.1f} us (min {us[1]:.1f}, max {us[2]:.1f})  "
                  f"{mb:6.1f} MB  {mb / us[0]:.2f} TB/s", flush=True)
    for nsd in (2, 3):
        for op in ("restrict", "prolong"):
            print(f"{nsd}-D {op}: general / nested = {rows[('general', nsd, op)] / rows[('nested', nsd, op)]:.2f}")


def timed_solve(label, sizes, B, **options):
    geom = geometry(sizes)
    g = torch.Generator().manual_seed(1)
    shape = (B, 1, *geom.node_shape)
    nu, f = (0.5 + torch.rand(shape, generator=g)).cuda(), torch.randn(shape, generator=g).cuda()
    jac = float(np.prod([0.5 * h for h in geom.hs]))
    kw = dict(nu=nu, f=f, dirichlet=[(BoxFaces("all"), 0.0)], jac=jac, tol=1e-5)
    solve.poisson_solve(geom, **kw, **{**options, "maxiter": 4})
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        u, info = solve.poisson_solve(geom, **kw, **options)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    R = ops.residual(geom, u, nu, f, None, kw["dirichlet"], jac).double().flatten(1).norm(dim=1).cpu().numpy() / np.sqrt(info.rr0)
    print(f"  {label:>34}: iterations {int(info.iterations.min())}..{int(info.iterations.max())}, converged {bool(info.converged.all())}, recurrence "
          f"{float(info.rel_residual.max()):.3e}, true |R| / |r0| {float(R.max()):.3e}, wall {sorted(times)[1] * 1e3:.1f} ms (min {min(times) * 1e3:.1f})", flush=True)


def convergence():
    import poisson_solve as ex
    general = dict(precondition="multigrid", mg_coarsening="general")
    for n, B in ((32, 1), (64, 1), (128, 1), (256, 1), (512, 1), (512, 16)):
        timed_solve(f"{n}^2 B={B} general multigrid", (n, n), B, **general)
        timed_solve(f"{n}^2 B={B} jacobi", (n, n), B, precondition="jacobi", maxiter=6000)
    timed_solve("513^2 B=16 nested multigrid", (513, 513), 16, precondition="multigrid")
    for n in (64, 128, 256):
        timed_solve(f"{n}^3 B=1 general multigrid", (n, n, n), 1, **general)
        timed_solve(f"{n}^3 B=1 jacobi", (n, n, n), 1, precondition="jacobi", maxiter=6000)
    timed_solve("257^3 B=1 nested multigrid", (257, 257, 257), 1, precondition="multigrid")
    ex.run_mms(128, 2, "multigrid", 1e-5, coarsening="general")
    ex.run_mms(128, 3, "multigrid", 1e-5, coarsening="general")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--transfers", action="store_true")
    ap.add_argument("--convergence", action="store_true")
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--replays", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mg_general.py measures on the GPU: no device visible")
    if a.transfers:
        transfers(a.iters, a.replays)
    if a.convergence:
        convergence()
