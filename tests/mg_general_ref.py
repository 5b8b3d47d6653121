"""Float64 restatement of the multigrid hierarchy on meshes that need not be nested (mg_coarsening="general" of diffnet_amd/solve.py,
csrc/poisson_mg_general.hip), numpy only, no GPU and nothing imported from the code under test but the plain-data FemGeometry.  The
cycle, M as a matrix and PCG are mg_ref's own (mg_ref.vcycle, mg_ref.preconditioner_matrix, mg_ref.pcg) on the level dicts built here:

  * the level shapes: an axis of e elements keeps ceil(e / 2) over the same length, while every axis has at least 3 elements;
  * the 1-D linear interpolation between two meshes over the same length from the integer rule (node i of the target at the source
    coordinate i (n_src - 1) / (n_dst - 1)), in float64 or with every weight rounded to float32, and its Kronecker products;
  * the levels: the same operator rediscretised on the level's shape and spacings with wscale = jac prod(hs_l / hs_0), nu interpolated
    multilinearly at the coarse nodes, the Dirichlet nodes those whose NEAREST fine node (per axis) is one, the inverse diagonal.

Dense: use it up to 64^2 and 16^3.  Arrays of one sample are flat in memory order (z, y, x), x fastest."""
import numpy as np

import mg_ref
import solve_ref
from diffnet_amd.fem import FemGeometry


def level_shapes(node_shape, max_levels=None):
    """Node shapes (memory order) of the levels."""
    shapes = [tuple(int(s) for s in node_shape)]
    while max_levels is None or len(shapes) < max_levels:
        nel = [s - 1 for s in shapes[-1]]
        if any(e < 3 for e in nel):
            break
        shapes.append(tuple(-(-e // 2) + 1 for e in nel))
    return shapes


def level_geometry(geom, shape):
    """The geometry of a level of node shape `shape` (memory order) over the box of `geom`."""
    sizes = tuple(shape[::-1])
    hs = tuple(h * (s0 - 1) / (s - 1) for h, s0, s in zip(geom.hs, geom.sizes, sizes))
    return FemGeometry(geom.nsd, sizes, hs, geom.deg, geom.ngp_1d, geom.gpx_1d, geom.gpw_1d)


def interp_1d(n_src, n_dst, rounded=False):
    """(n_dst, n_src): target node i lies at i (n_src - 1) / (n_dst - 1) = j + rem / (n_dst - 1) and takes (n_dst - 1 - rem) / (n_dst - 1)
    of source node j and rem / (n_dst - 1) of j + 1.  rounded: every weight rounded to float32 (the matrix stays float64)."""
    A = np.zeros((n_dst, n_src))
    for i in range(n_dst):
        j, rem = divmod(i * (n_src - 1), n_dst - 1)
        for col, w in ((j, (n_dst - 1 - rem) / (n_dst - 1)), (j + 1, rem / (n_dst - 1))):
            if w != 0:
                A[i, col] = np.float64(np.float32(w)) if rounded else w
    return A


def prolong_1d(nf, nc, rounded=False):
    """(nf, nc): the interpolation from the coarse to the fine nodes of one axis."""
    return interp_1d(nc, nf, rounded)


def kron_axes(mats):
    """The Kronecker product of per-axis matrices, slowest axis first: the operator on flat arrays in memory order."""
    A = np.ones((1, 1))
    for m in mats:
        A = np.kron(A, m)
    return A


def prolongation(fine_shape, coarse_shape, rounded=False):
    """P (n_fine, n_coarse) for flat arrays in memory order."""
    return kron_axes([prolong_1d(nf, nc, rounded) for nf, nc in zip(fine_shape, coarse_shape)])


def nearest_1d(nf, nc):
    """Per coarse node of an axis the nearest fine node (the lower of a tie): (2 j (nf - 1) + (nc - 1)) // (2 (nc - 1))."""
    return np.array([(2 * j * (nf - 1) + (nc - 1)) // (2 * (nc - 1)) for j in range(nc)])


def coarse_fixed(fixed, fine_shape, coarse_shape):
    a = np.asarray(fixed).reshape(fine_shape)
    for d, (nf, nc) in enumerate(zip(fine_shape, coarse_shape)):
        a = np.take(a, nearest_1d(nf, nc), axis=d)
    return a.ravel()


def coarse_nu(nu, fine_shape, coarse_shape):
    """nu interpolated multilinearly at the coarse nodes, float64."""
    return kron_axes([interp_1d(nf, nc) for nf, nc in zip(fine_shape, coarse_shape)]) @ np.asarray(nu, np.float64).ravel()


def hierarchy(geom, nu=None, fixed=None, jac=1.0, max_levels=None, rounded=False):
    """mg_ref's level dicts, fine first: dict(shape, K, fixed, dinv, P) with P the interpolation from the NEXT coarser level (None on
    the last).  rounded: P from the float32-rounded weights -- what a float32 run of the cycle multiplies by."""
    shapes = level_shapes(geom.node_shape, max_levels)
    n = int(np.prod(shapes[0]))
    nu_l = None if nu is None else np.asarray(nu, np.float64).ravel()
    fx_l = np.zeros(n, bool) if fixed is None else np.asarray(fixed).ravel().astype(bool)
    out = []
    for l, shp in enumerate(shapes):
        g = level_geometry(geom, shp)
        K = solve_ref.dense_stiffness(g, nu_l, jac * float(np.prod([hl / h0 for hl, h0 in zip(g.hs, geom.hs)])))
        last = l + 1 == len(shapes)
        out.append(dict(shape=shp, K=K, fixed=fx_l, dinv=solve_ref.dense_dinv(K, fx_l), P=None if last else prolongation(shp, shapes[l + 1], rounded)))
        if not last:
            nu_l = None if nu_l is None else coarse_nu(nu_l, shp, shapes[l + 1])
            fx_l = coarse_fixed(fx_l, shp, shapes[l + 1])
    return out


def with_rounded_weights(levels):
    """The same levels (K, dinv and fixed shared, not copied) with P from the float32-rounded weights."""
    out = []
    for l, L in enumerate(levels):
        M = {k: v for k, v in L.items() if not isinstance(k, tuple)}             # without mg_ref.vcycle's cache of cast matrices
        if L["P"] is not None:
            M["P"] = prolongation(L["shape"], levels[l + 1]["shape"], rounded=True)
        out.append(M)
    return out


vcycle, pcg, preconditioner_matrix = mg_ref.vcycle, mg_ref.pcg, mg_ref.preconditioner_matrix
