"""Float64 numpy restatement of the point-cloud terms on a Q1 mesh (diffnet_amd/points.py, csrc/point_terms.hip), written independently
of both: classify and clamp, the local coordinate, multilinear interpolation and its derivatives, the three penalty kinds with their
per-point cotangents, and the adjoint (a scatter, here with np.add.at in float64).  Axes are in the mesh's own order throughout:
axis 0 is x, the LAST tensor axis; callers map point columns to axes themselves."""
import numpy as np


def classify(points, hs, nel, dtype=np.float64):
    """points (N, nsd) with column d along mesh axis d (x first).  e = trunc(x / h) in `dtype` as the scripts do, clamped to the mesh;
    xi = 2 (x - e h) / h - 1 in float64.  Raises ValueError for a point outside [0, h nel] or a non-finite one."""
    pts = np.asarray(points)
    p64 = pts.astype(np.float64)
    nsd = p64.shape[1]
    e = np.empty(p64.shape, dtype=np.int64)
    xi = np.empty(p64.shape, dtype=np.float64)
    for d in range(nsd):
        L = hs[d] * nel[d] * (1.0 + 2.0 ** -50)
        if not np.all(np.isfinite(p64[:, d]) & (p64[:, d] >= 0.0) & (p64[:, d] <= L)):
            raise ValueError(f"a point lies outside [0, {L}] on axis {d}")
        q = pts[:, d].astype(dtype) / dtype(hs[d])
        e[:, d] = np.clip(np.trunc(q).astype(np.int64), 0, nel[d] - 1)
        xi[:, d] = 2.0 * (p64[:, d] - e[:, d] * hs[d]) / hs[d] - 1.0
    return e, xi


def flat_element(e, nel):
    """(ez nely + ey) nelx + ex"""
    f = np.zeros(e.shape[0], dtype=np.int64)
    for d in reversed(range(e.shape[1])):
        f = f * nel[d] + e[:, d]
    return f


def _corners(nsd):
    return [tuple((a >> d) & 1 for d in range(nsd)) for a in range(1 << nsd)]


def _weights(xi, corner, ds):
    """N_a and s_d d_d N_a (N,), (N, nsd) of the corner (0 / 1 per axis) at xi (N, nsd)"""
    nsd = xi.shape[1]
    w1 = [0.5 * (1.0 + (2 * corner[d] - 1) * xi[:, d]) for d in range(nsd)]
    d1 = [0.5 * (2 * corner[d] - 1) * np.ones(xi.shape[0]) for d in range(nsd)]
    N = np.prod(w1, axis=0)
    dN = np.stack([ds[d] * np.prod([d1[j] if j == d else w1[j] for j in range(nsd)], axis=0) for d in range(nsd)], 1)
    return N, dN


def _node_index(b, e, corner, sizes):
    """flat index into u (B, [nz,] ny, nx) of the corner node of element e in sample b"""
    nsd = e.shape[1]
    idx = b.astype(np.int64)
    for d in reversed(range(nsd)):
        idx = idx * sizes[d] + e[:, d] + corner[d]
    return idx


def interpolate(u, b, e, xi, ds):
    """u (B, [nz,] ny, nx) float64; per point: sample b, element e (N, nsd), local coordinate xi (N, nsd); ds: the derivative scales.
    Returns values (N), grads (N, nsd) and the sums of absolute terms the rounding bounds are stated in: sum_a |N_a u_a| (N) and
    s_d sum_a |d_d N_a u_a| (N, nsd)."""
    u = np.asarray(u, dtype=np.float64)
    sizes = u.shape[1:][::-1]
    uf = u.reshape(-1)
    nsd = e.shape[1]
    val, aval = np.zeros(len(b)), np.zeros(len(b))
    g, ag = np.zeros((len(b), nsd)), np.zeros((len(b), nsd))
    for c in _corners(nsd):
        N, dN = _weights(xi, c, ds)
        ua = uf[_node_index(b, e, c, sizes)]
        val += N * ua
        aval += np.abs(N * ua)
        g += dN * ua[:, None]
        ag += np.abs(dN * ua[:, None])
    return val, g, aval, ag


def penalty(val, g, target, normals, kind, w_val, w_nrm):
    """(value term, normals term, c0 (N), c (N, nsd)): the two weighted sums and the per-point cotangents of (u_p, g_d)"""
    dv = val - target
    lv = w_val * np.sum(dv ** 2)
    c0 = 2.0 * w_val * dv
    if kind == "none" or normals is None:
        return lv, 0.0, c0, np.zeros_like(g)
    if kind == "dot":
        r = np.sum(g * normals, 1) - 1.0
        return lv, w_nrm * np.sum(r ** 2), c0, 2.0 * w_nrm * r[:, None] * normals
    if kind == "match":
        r = g - normals
        return lv, w_nrm * np.sum(r ** 2), c0, 2.0 * w_nrm * r
    raise ValueError(kind)


def adjoint(shape, b, e, xi, c0, c, ds, gscale=1.0):
    """Pullback of the per-point cotangents to the nodes: grad (shape = (B, [nz,] ny, nx)), the bound's sum of absolute terms
    gscale sum_p (|c0 N_a| + sum_d |c_d s_d d_d N_a|) per node, and the number of points in the node's adjacent elements."""
    sizes = shape[1:][::-1]
    nsd = e.shape[1]
    n = int(np.prod(shape))
    grad, agrad, cnt = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    for corner in _corners(nsd):
        N, dN = _weights(xi, corner, ds)
        idx = _node_index(b, e, corner, sizes)
        np.add.at(grad, idx, gscale * (c0 * N + np.sum(c * dN, 1)))
        np.add.at(agrad, idx, abs(gscale) * (np.abs(c0 * N) + np.sum(np.abs(c * dN), 1)))
        np.add.at(cnt, idx, 1)
    return grad.reshape(shape), agrad.reshape(shape), cnt.reshape(shape)


def loss_and_grad(u, b, e, xi, ds, target, normals, kind, w_val=1.0, w_nrm=1.0):
    """(value term, normals term, grad) of the penalty at u"""
    val, g, _, _ = interpolate(u, b, e, xi, ds)
    lv, ln, c0, c = penalty(val, g, target, normals, kind, w_val, w_nrm)
    grad, _, _ = adjoint(np.asarray(u).shape, b, e, xi, c0, c, ds)
    return lv, ln, grad
