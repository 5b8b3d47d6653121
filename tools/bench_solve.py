#!/usr/bin/env python3
"""Measurements of the batched CG solve (diffnet_amd/solve.py; profiles/poisson_solve.txt).  Needs an MI355X.

    python tools/bench_solve.py [--shapes 512x512x1,512x512x16,1025x1025x1,128x128x128x1,256x256x256x1] [--iters 16] [--replays 30]
    python tools/bench_solve.py --trace 512x512x16        # a bare loop of iterations, for `rocprofv3 --kernel-trace --stats -- ...`
    python tools/bench_solve.py --convergence              # time to tol = 1e-5 (mms, CG against L-BFGS), Jacobi on a klsum field, stall level
    python tools/bench_solve.py --precondition multigrid [--shapes 513x513x16,1025x1025x1,129x129x129x1] [--trace ...] [--convergence]
                                                           # the same three modes for the multigrid preconditioner (profiles/poisson_multigrid.txt):
                                                           # one V-cycle and one preconditioned iteration, eager and as a HIP graph, beside one
                                                           # Jacobi iteration on the same shape; iterations and wall time to tol = 1e-5 against Jacobi

Per shape (nx x ny [x nz] x B; random nu in [0.5, 1.5], random f, u = 0 on the box faces, samples kept active with tol = 0):
  * device time per iteration: `--iters` iterations captured in one HIP graph, replayed `--replays` times after warm-up, timed by device events,
    median; the same for the operator launches alone; the three vector phases are the difference (per-kernel times: the --trace run);
  * the phases' bytes per second: 13 floats per node and iteration (the header comment of csrc/poisson_cg.hip) over their time, against the
    streaming probe of bench.py --full (dn_probe_stream: 3 reads + 1 write of 16 bytes per lane, best of its modes) run here over the
    solver's own arrays -- i.e. at the same footprint, which at the small shapes is cache-resident for both;
  * the same iteration composed from torch ops (PoissonSolver(phases="composed")), eager, host clock around a synchronised loop."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
from diffnet_amd import BoxFaces, _lib, ops, solve  # noqa: E402


def parse_shape(s):
    v = [int(x) for x in s.split("x")]
    return tuple(v[:-1]), v[-1]


def geometry(sizes):
    """unit square / cube, Q1, the 2-point rule (the plain description of the mesh: no host coordinate tables of a 256^3 module)"""
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    gx, gw = gauss_rule(2)
    return FemGeometry(len(sizes), tuple(sizes), tuple(1.0 / (s - 1) for s in sizes), 1, 2, gx, gw)


def make_solver(sizes, B, phases="fused", tol=0.0, precondition="jacobi"):
    geom = geometry(sizes)
    g = torch.Generator().manual_seed(1)
    shape = (B, 1, *geom.node_shape)
    nu = (0.5 + torch.rand(shape, generator=g)).cuda()
    f = torch.randn(shape, generator=g).cuda()
    jac = float(np.prod([0.5 * h for h in geom.hs]))
    return solve.PoissonSolver(geom, B, nu=nu, f=f, dirichlet=[(BoxFaces("all"), 0.0)], jac=jac, tol=tol, phases=phases, precondition=precondition)


def graph_median_us(body, iters, replays):
    """median device time of one `body()` call out of `iters` captured in a graph, over `replays` replays"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            body()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(iters):
                body()
        for _ in range(5):
            graph.replay()
        times = []
        for _ in range(replays):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            graph.replay()
            e1.record(side)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / iters)
    torch.cuda.current_stream().wait_stream(side)
    return statistics.median(times), min(times), max(times)


def probe_gbps(s, replays):
    """dn_probe_stream over the solver's arrays: best of the modes bench.py --full tries; bytes = 16 per node"""
    fn = _lib.lib().dn_probe_stream
    n = (s.x.numel() // 4) * 4
    best = None
    for mode in (0, 1, 4, 5, 8, 9, 7):
        def body():
            rc = fn(s.x.data_ptr(), s.r.data_ptr(), s.p.data_ptr(), s.q.data_ptr(), n, mode, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            if rc:
                raise RuntimeError(f"dn_probe_stream rc={rc}")
        us = graph_median_us(body, 16, replays)[0]
        if best is None or us < best[0]:
            best = (us, mode)
    return 16.0 * n / (best[0] * 1e-6) / 1e9, best[1], best[0]


def bench_shape(sizes, B, iters, replays):
    s = make_solver(sizes, B).setup()
    n = s.n * B
    s.iterate(4)
    it = graph_median_us(lambda: s.iterate(1), iters, replays)
    s.setup()
    op = graph_median_us(s._plan.launch, iters, replays)
    # the three phases: the iteration less its operator launch (their launch gaps included).  They cannot be replayed alone: without the
    # operator between them q goes stale, p q turns negative and the sample breaks down -- after which the phases skip it
    ph = (it[0] - op[0],)
    ph_gbps = 13 * 4.0 * n / (ph[0] * 1e-6) / 1e9
    s.setup()
    pr_gbps, mode, pr_us = probe_gbps(s, replays)
    st = s.status()
    assert st.active.all(), "the samples must stay active while they are timed"
    # composed, eager
    c = make_solver(sizes, B, phases="composed").setup()
    c.iterate(3)
    torch.cuda.synchronize()
    reps = []
    for _ in range(5):
        t0 = time.perf_counter()
        c.iterate(8)
        torch.cuda.synchronize()
        reps.append((time.perf_counter() - t0) / 8 * 1e6)
    comp = statistics.median(reps)
    name = "x".join(map(str, sizes)) + f" B={B}"
    print(f"{name:>22}: iteration {it[0]:8.1f} us (min {it[1]:.1f}, max {it[2]:.1f})  operator {op[0]:7.1f}  phases {ph[0]:7.1f} "
          f"= {ph_gbps:6.0f} GB/s | probe {pr_gbps:6.0f} GB/s (mode {mode}, {pr_us:.1f} us) ratio {ph_gbps / pr_gbps:.2f} | "
          f"composed eager {comp:8.1f} us = {comp / it[0]:.1f} x", flush=True)


def eager_us(body, k=8, reps=5):
    """median host-clock time of one `body()` out of k in a synchronised loop"""
    body()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(k):
            body()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / k * 1e6)
    return statistics.median(out)


def bench_shape_multigrid(sizes, B, iters, replays):
    """One V-cycle and one multigrid-preconditioned iteration, eager and captured, beside one Jacobi iteration on the same shape."""
    name = "x".join(map(str, sizes)) + f" B={B}"
    s = make_solver(sizes, B, precondition="multigrid").setup()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nl, launches = len(s.mg.levels), len(s.mg._seq)
    s.iterate(2)
    it_e = eager_us(lambda: s.iterate(1))
    s.setup()
    it = graph_median_us(lambda: s.iterate(1), iters, replays)
    assert s.status().active.all(), "the samples must stay active while they are timed"
    s.setup()
    vc_e = eager_us(lambda: s.mg.launch(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    vc = graph_median_us(lambda: s.mg.launch(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), iters, replays)
    j = make_solver(sizes, B).setup()
    j.iterate(2)
    jt_e = eager_us(lambda: j.iterate(1))
    j.setup()
    jt = graph_median_us(lambda: j.iterate(1), iters, replays)
    print(f"{name:>22}: {nl} levels, {launches} launches per V-cycle | V-cycle graph {vc[0]:8.1f} us (min {vc[1]:.1f}, max {vc[2]:.1f}) eager {vc_e:8.1f} | "
          f"multigrid iteration graph {it[0]:8.1f} us (min {it[1]:.1f}, max {it[2]:.1f}) eager {it_e:8.1f} | "
          f"Jacobi iteration graph {jt[0]:7.1f} us eager {jt_e:7.1f} | one multigrid iteration = {it[0] / jt[0]:.1f} Jacobi iterations (graph), {it_e / jt_e:.1f} (eager)",
          flush=True)


def timed_solve(label, geom, precondition, **kw):
    """iterations and wall time of one solve to tol = 1e-5 (after an untimed first call) and the true relative residual at the end"""
    solve.poisson_solve(geom, precondition=precondition, tol=1e-5, **{**kw, "maxiter": 4})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u, info = solve.poisson_solve(geom, precondition=precondition, tol=1e-5, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    R = ops.residual(geom, u, kw.get("nu"), kw.get("f"), None, kw["dirichlet"], kw["jac"]).double()
    print(f"  {label} precondition {precondition}: {int(info.iterations[0])} iterations, converged {bool(info.converged[0])}, recurrence "
          f"{float(info.rel_residual[0]):.3e}, true |R| / |r0| {float(R.norm()) / float(np.sqrt(info.rr0[0])):.3e}, wall {dt * 1e3:.1f} ms", flush=True)


def convergence_multigrid():
    """Iterations and wall time to tol = 1e-5, multigrid against Jacobi: the klsum 257^2 case and the 1025^2 random-coefficient case of
    profiles/poisson_solve.txt, break-even over the mesh size, the compliance example."""
    import poisson_solve as ex
    from diffnet_amd.gen_input_calc import generate_diffusivity_tensor
    n = 257
    geom = geometry((n, n))
    nu = torch.from_numpy(np.ascontiguousarray(generate_diffusivity_tensor([1.2, -0.8, 1.5, 0.6, -1.1, 0.9], n), dtype=np.float32))[None].cuda()
    jac = float(np.prod([0.5 * h for h in geom.hs]))
    dl = [(BoxFaces("xlo"), 1.0), (BoxFaces("xhi"), 0.0)]
    print(f"klsum {n}^2: nu in [{float(nu.min()):.3f}, {float(nu.max()):.3f}]")
    for pre in ("multigrid", "jacobi"):
        timed_solve(f"klsum {n}^2", geom, pre, nu=nu, dirichlet=dl, jac=jac, maxiter=40 * n)
    for n in (33, 65, 129, 257, 513, 1025):
        geom = geometry((n, n))
        g = torch.Generator().manual_seed(1)
        shape = (1, 1, n, n)
        nu, f = (0.5 + torch.rand(shape, generator=g)).cuda(), torch.randn(shape, generator=g).cuda()
        jac = float(np.prod([0.5 * h for h in geom.hs]))
        for pre in ("multigrid", "jacobi"):
            timed_solve(f"random nu {n}^2", geom, pre, nu=nu, f=f, dirichlet=[(BoxFaces("all"), 0.0)], jac=jac, maxiter=6000)
    for pre in ("multigrid", "jacobi"):
        ex.run_compliance(65, 8, "fused", precondition=pre)


def trace(sizes, B, iters=200, precondition="jacobi"):
    s = make_solver(sizes, B, precondition=precondition).setup()
    s.iterate(iters)
    torch.cuda.synchronize()
    print("trace loop done:", "x".join(map(str, sizes)), "B", B, "iterations", iters)


def convergence():
    import poisson_solve as ex
    for n in (129, 257):
        ex.run_mms(n, 2, "jacobi", 1e-5, "lbfgs")
    ex.run_mms(65, 3, "jacobi", 1e-5)
    # Jacobi against none on a klsum coefficient field (nu = exp(KL sum), the reference's 12_klsum.py family), u = 1 / 0 on the x faces
    from diffnet_amd.gen_input_calc import generate_diffusivity_tensor
    n = 257
    geom = geometry((n, n))
    nu = torch.from_numpy(np.ascontiguousarray(generate_diffusivity_tensor([1.2, -0.8, 1.5, 0.6, -1.1, 0.9], n), dtype=np.float32))[None].cuda()
    jac = float(np.prod([0.5 * h for h in geom.hs]))
    dl = [(BoxFaces("xlo"), 1.0), (BoxFaces("xhi"), 0.0)]
    print(f"klsum {n}^2: nu in [{float(nu.min()):.3f}, {float(nu.max()):.3f}]")
    for pre in ("jacobi", None):
        u, info = solve.poisson_solve(geom, nu=nu, dirichlet=dl, jac=jac, tol=1e-5, precondition=pre, maxiter=40 * n)
        print(f"  precondition {pre}: {int(info.iterations[0])} iterations, converged {bool(info.converged[0])}, relative residual {float(info.rel_residual[0]):.3e}")
    # where float32 CG stalls: the smallest relative TRUE residual reached at 1025^2 (recurrence driven far below it)
    n = 1025
    s = make_solver((n, n), 1, tol=1e-9)
    s.setup()
    best, done = None, 0
    while done < 6000:
        s.iterate(500)
        done += 500
        R = ops.residual(s.geom, s.x, s.nu, s.f, None, s.dl, s.jac).double()
        st = s.status()
        true_rel = float(R.norm()) / float(np.sqrt(st.rr0[0]))
        print(f"  1025^2 after {done} iterations: recurrence {float(st.rel_residual[0]):.3e}  true |R| / |r0| {true_rel:.3e}")
        best = true_rel if best is None else min(best, true_rel)
        if not st.active.any():
            break
    print(f"1025^2: float32 CG stalls at a relative true residual of about {best:.1e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x512x1,512x512x16,1025x1025x1,128x128x128x1,256x256x256x1")
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--convergence", action="store_true")
    ap.add_argument("--precondition", choices=("jacobi", "multigrid"), default="jacobi")
    a = ap.parse_args()
    mg = a.precondition == "multigrid"
    if not torch.cuda.is_available():
        raise SystemExit("bench_solve.py measures on the GPU: no device visible")
    if a.trace:
        trace(*parse_shape(a.trace), iters=40 if mg else 200, precondition=a.precondition)
    elif a.convergence:
        convergence_multigrid() if mg else convergence()
    else:
        print(torch.cuda.get_device_name(0), _lib.lib().dn_build_info().decode())
        for sh in a.shapes.split(","):
            (bench_shape_multigrid if mg else bench_shape)(*parse_shape(sh), a.iters, a.replays)
