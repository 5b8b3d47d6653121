#!/usr/bin/env python3
"""The discrete solution the Poisson losses converge to, solved directly: batched preconditioned CG on the fused operator
(diffnet_amd/solve.py, dn_poisson_diag + dn_poisson_cg; --precondition multigrid: a geometric multigrid V-cycle per iteration,
dn_poisson_mg + dn_poisson_pcg, on meshes of k 2^(L-1) + 1 nodes per axis; --coarsening general: on any mesh with at least 3 elements per
axis, dn_poisson_mg_transfer where a level is not nested) instead of an optimiser on the loss.  Q1 meshes only.

    python examples/poisson_solve.py --case mms [--n 129] [--nsd 2|3] [--precondition jacobi|multigrid|none] [--coarsening nested|general] [--tol 1e-5] [--compare lbfgs]
    python examples/poisson_solve.py --case ibn [--n 33] [--points 2000] [--precondition jacobi|multigrid]
    python examples/poisson_solve.py --case compliance [--n 65] [--steps 8] [--mode fused|composed] [--precondition jacobi|multigrid]

mms         the manufactured problems of the reference's e8_2d_poisson_mms.py / e8_3d_poisson_mms.py (u = prod sin(pi x_d), f = nsd pi^2 u,
            u = 0 on the boundary): iterations, relative residual, the calc_l2_err figures, wall time.  --compare lbfgs also runs the
            route of examples/poisson_2d_energy.py (L-BFGS on the energy loss) until it reaches the energy of the CG solution.
ibn         the winding-number mask of a point cloud as the Dirichlet source (u = 1), the box faces as the sink (u = 0), as in
            examples/ibn_3d_pointcloud.py, solved directly: there is no analytical solution to compare with, which is the point.
compliance  a few steps of NESTED compliance minimisation over a nodal density rho: nu = 0.001 + sigmoid(rho)^3, loss = sum f u*(nu),
            differentiated through the solve (implicit function: one more solve, one dn_poisson_coef_grad launch).  No volume constraint:
            the steps show the gradient at work (material goes where it lowers the compliance most), not a design.
            --mode selects the solver's vector phases: fused = the dn_poisson_cg kernels, composed = the same recurrences from torch ops."""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from diffnet_amd import BoxFaces, DiffNet2DFEM, DiffNet3DFEM  # noqa: E402


class Mms2D(DiffNet2DFEM):
    def exact_solution(self, x, y):
        return torch.sin(math.pi * x) * torch.sin(math.pi * y)


class Mms3D(DiffNet3DFEM):
    def exact_solution(self, x, y, z):
        return torch.sin(math.pi * x) * torch.sin(math.pi * y) * torch.sin(math.pi * z)


def run_mms(n=129, nsd=2, precondition="jacobi", tol=1e-5, compare=None, verbose=True, coarsening="nested"):
    dev = torch.device("cuda")
    m = (Mms2D if nsd == 2 else Mms3D)(None, None, domain_size=n, nsd=nsd)
    coords = (m.xx, m.yy) if nsd == 2 else (m.xx, m.yy, m.zz)
    u_exact = m.exact_solution(*coords)
    f = (nsd * math.pi ** 2 * u_exact)[None, None].float().contiguous().to(dev)
    jac = float(np.prod([0.5 * h for h in m.geom.hs]))
    bc = [(BoxFaces("all"), 0.0)]
    m.solve(f=f, dirichlet=bc, jac=jac, tol=tol, maxiter=8, precondition=precondition, mg_coarsening=coarsening)      # first-call set-up (kernel load) outside the timing
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u, info = m.solve(f=f, dirichlet=bc, jac=jac, tol=tol, precondition=precondition, mg_coarsening=coarsening)
    torch.cuda.synchronize()
    t_cg = time.perf_counter() - t0
    eL2, uL2, exL2 = (float(v) for v in m._l2_terms(u))                  # the sums of calc_l2_err, without its prints
    out = dict(iterations=int(info.iterations[0]), rel_residual=float(info.rel_residual[0]), converged=bool(info.converged[0]),
               eL2=eL2, rel_eL2=eL2 / exL2, seconds=t_cg)
    if verbose:
        print(f"mms {nsd}-D n = {n}  precondition {precondition}  tol {tol:g}: converged {out['converged']} after {out['iterations']} iterations, "
              f"relative residual {out['rel_residual']:.3e}")
        print(f"  ||e||_L2 = {eL2:.4e}  ||u||_L2 = {uL2:.4e}  ||u_ex||_L2 = {exL2:.4e}  relative {out['rel_eL2']:.3e}  (h^2 = {m.geom.hs[0] ** 2:.3e})")
        print(f"  wall time {t_cg * 1e3:.2f} ms")
    if compare == "lbfgs":
        if nsd != 2:
            raise ValueError("--compare lbfgs follows examples/poisson_2d_energy.py: 2-D only")
        e_cg = float(m.energy_loss(u, None, f, dirichlet=bc, c=0.5, jac=jac))
        p = torch.nn.Parameter(torch.zeros_like(u))
        # the optimiser of examples/poisson_2d_energy.py; its default gradient / change tolerances (1e-7, 1e-9) are absolute and the mean
        # energy of a fine mesh has a smaller gradient than that from the start, so they are switched off
        opt = torch.optim.LBFGS([p], lr=1.0, max_iter=20, tolerance_grad=0.0, tolerance_change=0.0, line_search_fn="strong_wolfe")

        def closure():
            opt.zero_grad(set_to_none=True)
            val = m.energy_loss(p, None, f, dirichlet=bc, c=0.5, jac=jac)
            val.backward()
            return val

        float(closure())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        epochs, e = 0, float("inf")
        while epochs < 400 and not e <= e_cg + 1e-6 * abs(e_cg):
            e = float(opt.step(closure))
            epochs += 1
        torch.cuda.synchronize()
        t_lb = time.perf_counter() - t0
        out.update(lbfgs_seconds=t_lb, lbfgs_epochs=epochs, lbfgs_energy=e, cg_energy=e_cg)
        if verbose:
            print(f"  L-BFGS on the energy loss: {epochs} epochs of 20 to energy {e:.8f} (CG solution {e_cg:.8f}), wall time {t_lb * 1e3:.1f} ms "
                  f"= {t_lb / t_cg:.1f} x the CG solve")
    return out


def run_ibn(n=33, npts=2000, tol=1e-5, verbose=True, precondition="jacobi", coarsening="nested"):
    from ibn_3d_pointcloud import ellipsoid_cloud
    from diffnet_amd.winding import winding_mask
    dev = torch.device("cuda")
    m = DiffNet3DFEM(None, None, domain_size=n, nsd=3)
    pts, nrm, area = ellipsoid_cloud(npts, (0.3, 0.3, 0.3))
    nodes = torch.stack((m.xx, m.yy, m.zz)).to(dev)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None].to(dev)      # noqa: E731
    source = winding_mask(f32(pts), f32(nrm), f32(area), nodes)                 # uint8 (1, 1, n, n, n)
    t0 = time.perf_counter()
    u, info = m.solve(dirichlet=[(source, 1.0), (BoxFaces("all"), 0.0)], tol=tol, precondition=precondition, mg_coarsening=coarsening)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    energy = float(m.energy_loss(u, None, None, dirichlet=[(source, 1.0), (BoxFaces("all"), 0.0)], c=0.5))
    if verbose:
        print(f"ibn n = {n}^3, {int(source.sum())} source nodes: converged {bool(info.converged[0])} after {int(info.iterations[0])} iterations, "
              f"relative residual {float(info.rel_residual[0]):.3e}, energy {energy:.6f}, u in [{float(u.min()):.4f}, {float(u.max()):.4f}], "
              f"{dt * 1e3:.1f} ms")
    return dict(converged=bool(info.converged[0]), iterations=int(info.iterations[0]), energy=energy, umin=float(u.min()), umax=float(u.max()))


def run_compliance(n=65, steps=8, mode="fused", lr=0.5, verbose=True, precondition="jacobi", coarsening="nested"):
    dev = torch.device("cuda")
    m = DiffNet2DFEM(None, None, domain_size=n)
    jac = float(np.prod([0.5 * h for h in m.geom.hs]))
    f = torch.zeros(1, 1, n, n, device=dev)
    f[..., n // 2 - 2:n // 2 + 3, -6:-1] = 1.0                                   # a heated patch near the right edge
    sink = BoxFaces("xlo")                                                      # u = 0 on the left edge
    rho = torch.zeros(1, 1, n, n, device=dev, requires_grad=True)
    opt = torch.optim.Adam([rho], lr=lr)
    hist = []
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        dens = torch.sigmoid(rho)
        nu = 0.001 + dens ** 3
        u, info = m.solve(nu=nu, f=f, dirichlet=[(sink, 0.0)], jac=jac, tol=1e-5, maxiter=100 * n, phases=mode,
                          precondition=precondition, mg_coarsening=coarsening)
        compliance = (f * u).sum()
        compliance.backward()
        opt.step()
        hist.append((float(compliance.detach()), float(dens.detach().mean()), int(info.iterations[0]), bool(info.converged[0]),
                     int(info.adjoint.iterations[0])))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if verbose:
        for k, (cval, vol, its, ok, adj) in enumerate(hist):
            print(f"compliance [{mode}, {precondition}] step {k}: sum f u* = {cval:.6f}  volume {vol:.3f}  {its} iterations (adjoint {adj})  converged {ok}")
        print(f"compliance [{mode}, {precondition}]: {hist[0][0]:.6f} -> {hist[-1][0]:.6f} in {steps} steps, {dt:.2f} s")
    return hist


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("mms", "ibn", "compliance"), default="mms")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--nsd", type=int, default=2)
    ap.add_argument("--precondition", choices=("jacobi", "multigrid", "none"), default="jacobi")
    ap.add_argument("--coarsening", choices=("nested", "general"), default="nested")
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--compare", choices=("lbfgs",), default=None)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    a = ap.parse_args()
    if a.case == "mms":
        run_mms(a.n or 129, a.nsd, None if a.precondition == "none" else a.precondition, a.tol, a.compare, coarsening=a.coarsening)
    elif a.case == "ibn":
        run_ibn(a.n or 33, a.points, a.tol, precondition=None if a.precondition == "none" else a.precondition, coarsening=a.coarsening)
    else:
        run_compliance(a.n or 65, a.steps, a.mode, precondition=None if a.precondition == "none" else a.precondition, coarsening=a.coarsening)
