"""Float64 restatement of the multigrid-preconditioned CG solve (diffnet_amd/solve.py, csrc/poisson_mg.hip, dn_poisson_pcg), numpy only,
no GPU and nothing imported from the code under test but the plain-data FemGeometry:

  * the explicit multilinear interpolation matrices P between nested meshes;
  * the levels of a hierarchy: the same operator rediscretised (tests/solve_ref.dense_stiffness on a geometry with halved element
    counts and doubled spacings, wscale = jac 2^(nsd l)), nu and the Dirichlet nodes injected (every second node), the inverse diagonal;
  * the V-cycle z = M r as dense algebra, statement by statement as solve.py launches it, in float64 or in float32;
  * M as a matrix, column by column;
  * PCG with it, in the structure of solve_ref.cg_restated (float64, or float32 with float64 dot products and float32 alpha / beta).

Dense: use it up to 65^2 and 17^3.  Arrays of one sample are flat in memory order (z, y, x), x fastest."""
import numpy as np

import solve_ref
from diffnet_amd.fem import FemGeometry


def level_shapes(node_shape, max_levels=None):
    """Node shapes (memory order) of the levels: coarsen while every axis has an even element count and the coarse mesh keeps at
    least 2 elements per axis."""
    shapes = [tuple(int(s) for s in node_shape)]
    while max_levels is None or len(shapes) < max_levels:
        nel = [s - 1 for s in shapes[-1]]
        if any(e % 2 or e // 2 < 2 for e in nel):
            break
        shapes.append(tuple(e // 2 + 1 for e in nel))
    return shapes


def level_geometry(geom, l):
    """The geometry of level l: the same rule, element counts halved l times, spacings doubled l times."""
    sizes = tuple((s - 1) // 2 ** l + 1 for s in geom.sizes)
    return FemGeometry(geom.nsd, sizes, tuple(h * 2 ** l for h in geom.hs), geom.deg, geom.ngp_1d, geom.gpx_1d, geom.gpw_1d)


def prolong_1d(nc):
    """(2 nc - 1, nc): fine node 2 i takes coarse node i, fine node 2 i + 1 half of i and half of i + 1."""
    P = np.zeros((2 * nc - 1, nc))
    for i in range(nc):
        P[2 * i, i] = 1.0
        if i + 1 < nc:
            P[2 * i + 1, i] = P[2 * i + 1, i + 1] = 0.5
    return P


def prolongation(coarse_shape):
    """P (n_fine, n_coarse) for flat arrays in memory order: the Kronecker product of the per-axis matrices, slowest axis first."""
    P = np.ones((1, 1))
    for nc in coarse_shape:
        P = np.kron(P, prolong_1d(nc))
    return P


def inject(a, shape):
    """Every second node of a nodal array of `shape` (flat or shaped), flat."""
    a = np.asarray(a).reshape(shape)
    return a[tuple(slice(None, None, 2) for _ in shape)].ravel()


def hierarchy(geom, nu=None, fixed=None, jac=1.0, max_levels=None):
    """The levels, fine first: dict(shape, K, fixed, dinv, P) with P the interpolation from the NEXT coarser level (None on the last).
    nu: nodal array of the fine mesh or None; fixed: bool array of the fine mesh's Dirichlet nodes (the union of the conditions)."""
    shapes = level_shapes(geom.node_shape, max_levels)
    n = int(np.prod(shapes[0]))
    nu_l = None if nu is None else np.asarray(nu, np.float64).ravel()
    fx_l = np.zeros(n, bool) if fixed is None else np.asarray(fixed).ravel().astype(bool)
    out = []
    for l, shp in enumerate(shapes):
        K = solve_ref.dense_stiffness(level_geometry(geom, l), nu_l, jac * 2.0 ** (geom.nsd * l))
        out.append(dict(shape=shp, K=K, fixed=fx_l, dinv=solve_ref.dense_dinv(K, fx_l), P=prolongation(shapes[l + 1]) if l + 1 < len(shapes) else None))
        if l + 1 < len(shapes):
            nu_l = None if nu_l is None else inject(nu_l, shp)
            fx_l = inject(fx_l, shp)
    return out


def vcycle(levels, r, sweeps=1, omega=0.8, coarse_sweeps=4, dtype=np.float64, l=0):
    """z = M r: SMOOTH0, sweeps - 1 more sweeps, restriction of the residual, the coarser levels, the interpolated correction, `sweeps`
    sweeps; on the last level `coarse_sweeps` sweeps from zero.  Every statement rounds to `dtype`."""
    L = levels[l]
    cast = L.setdefault(("cast", np.dtype(dtype).name), {})           # the level's matrices in `dtype`, converted once
    for k in ("K", "dinv", "P"):
        if k not in cast and L[k] is not None:
            cast[k] = L[k].astype(dtype)
    K, fx, dv = cast["K"], L["fixed"], cast["dinv"]
    om = dtype(omega)
    b = np.asarray(r).astype(dtype)
    op = lambda v: np.where(fx, 0, K @ v).astype(dtype)
    smooth = lambda x: (x + (om * dv) * (b - op(x))).astype(dtype)
    x = (om * dv * b).astype(dtype)
    last = l + 1 == len(levels)
    for _ in range((coarse_sweeps if last else sweeps) - 1):
        x = smooth(x)
    if last:
        return x
    P = cast["P"]
    bc = np.where(levels[l + 1]["fixed"], 0, P.T @ (b - op(x))).astype(dtype)
    ec = vcycle(levels, bc, sweeps, omega, coarse_sweeps, dtype, l + 1)
    x = (x + np.where(fx, 0, P @ ec)).astype(dtype)
    for _ in range(sweeps):
        x = smooth(x)
    return x


def preconditioner_matrix(levels, **kw):
    """M, column by column."""
    n = levels[0]["K"].shape[0]
    return np.stack([vcycle(levels, e, **kw) for e in np.eye(n)], axis=1)


def pcg(K, b, conditions=(), x0=None, levels=None, tol=1e-5, atol=0.0, maxiter=1000, dtype=np.float64, extra_load=None, **mg):
    """dn_poisson_pcg's recurrences for one sample in `dtype` with z = vcycle(levels, r): the structure of solve_ref.cg_restated.
    Returns (x, info) with info = dict(iterations, rr, rr0, converged, breakdown, active, r)."""
    n = len(b)
    fx = solve_ref.fixed_nodes(n, conditions)
    Kd, bd = K.astype(dtype), b.astype(dtype)
    if extra_load is not None:
        bd = bd + np.where(fx, 0, extra_load).astype(dtype)
    op = lambda v: np.where(fx, 0, Kd @ v).astype(dtype)
    M = lambda v: vcycle(levels, v, dtype=dtype, **mg).astype(dtype)
    dot = solve_ref._dot64
    t2, a2 = np.float64(np.float32(tol)) ** 2, np.float64(np.float32(atol)) ** 2
    # RESID0
    x = solve_ref.substitute(np.zeros(n) if x0 is None else x0, conditions).astype(dtype)
    r = (-np.where(fx, 0, Kd @ x - bd)).astype(dtype)
    rr0 = rr = dot(r, r)
    rz = 0.0
    active, its, breakdown = rr0 > a2, 0, not (rr0 == rr0)
    p = np.zeros(n, dtype)
    while active:
        # the V-cycle, RZ, DIRECTION
        z = M(r)
        rzn = dot(r, z)
        beta = dtype(rzn / rz) if rz > 0 else dtype(0)
        rz = rzn
        p = z if beta == 0 else (z + beta * p).astype(dtype)
        if its >= maxiter:
            break
        q = op(p)
        # DOT
        pq = dot(p, q)
        if not pq > 0:
            breakdown, active = True, False
            break
        alpha = dtype(rz / pq)
        # UPDATE
        x = (x + alpha * p).astype(dtype)
        r = (r - alpha * q).astype(dtype)
        rr = dot(r, r)
        its += 1
        active = rr > max(t2 * rr0, a2)
        if not rr == rr:
            breakdown = True
    conv = (not active) and (not breakdown) and rr <= max(t2 * rr0, a2)
    return x.astype(np.float64), dict(iterations=its, rr=rr, rr0=rr0, converged=conv, breakdown=breakdown, active=bool(active),
                                   r=r.astype(np.float64))
