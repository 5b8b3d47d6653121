"""Winding-number fields and inside/outside masks of point clouds with normals and areas, 2-D and 3-D, on one HIP launch
(ops.winding_field -> dn_winding_field).

    compute_winding_torch   drop-in for the reference's 3-D function of that name (L1 distance cubed, no constant, swapped axes)
    winding_number          the true generalised winding number (Euclidean distance, power = dim, 1/(2 pi) or 1/(4 pi)), mesh order
    winding_mask            its thresholded mask, straight from the kernel, ready as a Dirichlet mask of the fused operators
    read_xyzna              the reference's text format of a cloud: points, normals, areas

    winding_field_ad        the flat field (B, nq) with a fused backward pass (ops.winding_field_vjp -> dn_winding_field_vjp) with
                            respect to points, normals and area; queries are constants
    winding_field_composed  the same sum in plain torch, chunked over the queries: any device and dtype, differentiable by autograd in
                            every argument (queries included) and to any order -- the route for CPU tensors, float64, query
                            gradients and double backward

By default nothing is recorded for autograd, as before: the reference only thresholds the field, and inputs that require grad are used
detached.  `compute_winding_torch(..., differentiable=True)` and `winding_number(..., differentiable=True)` attach the result to the
graph with respect to points, normals and area (the reference's compute_winding_torch is plain torch, hence differentiable, and the
file that holds it is named for that).  The backward pass is one fused launch (two when the query range is split) that saves only the
inputs; it is once differentiable.  winding_mask stays non-differentiable.
"""
import math

import numpy as np
import torch

from . import ops


def _cloud(points, normals, area, detach=True):
    """(B, Np, dim) points and normals, (B, Np) area or None, contiguous and (unless detach is off) detached"""
    for name, t in (("points", points), ("normals", normals)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[-1] not in (2, 3):
            raise ValueError(f"{name} must be a tensor (B, Np, 2) or (B, Np, 3), got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    if normals.shape != points.shape:
        raise ValueError(f"normals {tuple(normals.shape)} do not match points {tuple(points.shape)}")
    if area is not None:
        if not isinstance(area, torch.Tensor) or tuple(area.shape) not in (tuple(points.shape[:2]), tuple(points.shape[:2]) + (1,)):
            raise ValueError(f"area must be None or a tensor (B, Np) or (B, Np, 1) for points {tuple(points.shape)}")
        area = (area.detach() if detach else area).reshape(points.shape[0], points.shape[1]).contiguous()
    if not detach:
        return points.contiguous(), normals.contiguous(), area
    return points.detach().contiguous(), normals.detach().contiguous(), area


class _WindingField(torch.autograd.Function):
    """ops.winding_field with ops.winding_field_vjp as its backward pass; saves the inputs only, never the field"""

    @staticmethod
    def forward(ctx, points, normals, area, queries, metric, power, scale, tile, slices):
        w, _ = ops.winding_field(points, normals, area, queries, metric=metric, power=power, scale=scale, tile=tile)
        ctx.save_for_backward(points, normals, area, queries)
        ctx.conf = (metric, power, scale, slices)
        return w

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        points, normals, area, queries = ctx.saved_tensors
        metric, power, scale, slices = ctx.conf
        want = tuple(name for name, need in zip(("points", "normals", "area"), ctx.needs_input_grad[:3]) if need)
        gp = gn = ga = None
        if want:
            gp, gn, ga = ops.winding_field_vjp(points, normals, area, queries, grad.contiguous(), metric=metric, power=power, scale=scale,
                                               want=want, slices=slices)
        return gp, gn, ga, None, None, None, None, None, None


def _no_query_grad(queries):
    if isinstance(queries, torch.Tensor) and queries.requires_grad:
        raise ValueError("the fused winding-number field has no gradient with respect to the queries: detach them, or use the composed "
                         "route diffnet_amd.winding.winding_field_composed, which differentiates every argument")


def winding_field_ad(points, normals, area, queries, metric, power, scale, tile=0, slices=0):
    """ops.winding_field's field (B, nq), attached to the autograd graph with respect to points, normals and area (each float32,
    contiguous, on the GPU; area (B, Np), (B, Np, 1) or None).  The backward pass is ops.winding_field_vjp, asked only for the inputs
    that need a gradient; it is once differentiable.  Queries are constants: a query tensor that requires grad is rejected (use
    winding_field_composed).  tile, slices: as in ops.winding_field and ops.winding_field_vjp."""
    _no_query_grad(queries)
    return _WindingField.apply(points, normals, area, queries, metric, power, scale, tile, slices)


def winding_field_composed(points, normals, area, queries, metric, power, scale, tile=0, slices=0, chunk=4096):
    """The sum of ops.winding_field in plain torch, `chunk` queries at a time:
        w[b, q] = scale sum_p area_p ((x_p - q) . n_p) / dist(x_p - q)^power,    dist the L1 ("l1") or the Euclidean ("l2") norm
    for any device and floating dtype, differentiable by autograd in every tensor argument, queries included, and to any order.
    points, normals (B, Np, dim); area (B, Np), (B, Np, 1) or None; queries (dim, nq) or (dim, *grid); returns (B, nq).  tile and
    slices are accepted for a common signature with winding_field_ad and ignored.  Peak memory is B x chunk x Np x dim values (and as
    much again per chunk for the graph)."""
    if metric not in ("l1", "l2"):
        raise ValueError(f"metric must be 'l1' or 'l2', got {metric!r}")
    if points.dim() != 3 or normals.shape != points.shape or queries.dim() < 2 or queries.shape[0] != points.shape[-1]:
        raise ValueError(f"points, normals (B, Np, dim) and queries (dim, ...) expected, got {tuple(points.shape)}, {tuple(normals.shape)}, "
                         f"{tuple(queries.shape)}")
    q_all = queries.reshape(queries.shape[0], -1)
    an = normals if area is None else normals * area.reshape(points.shape[0], points.shape[1], 1)
    out = []
    for q0 in range(0, q_all.shape[1], chunk):
        d = points[:, None, :, :] - q_all[:, q0:q0 + chunk].T[None, :, None, :]                # (B, nqc, Np, dim)
        dist = d.abs().sum(-1) if metric == "l1" else torch.sqrt((d * d).sum(-1))
        out.append(((d * an[:, None, :, :]).sum(-1) / dist ** power).sum(-1))
    return scale * torch.cat(out, 1)


def _grid_queries(queries, dim):
    """queries (dim, *grid) in mesh order (x the last axis) -> the tensor itself, detached and contiguous, and the grid shape"""
    if not isinstance(queries, torch.Tensor) or queries.dim() != dim + 1 or queries.shape[0] != dim:
        want = "(2, Ny, Nx)" if dim == 2 else "(3, Nz, Ny, Nx)"
        raise ValueError(f"queries must be a tensor {want} for {dim}-D points, got {tuple(queries.shape) if isinstance(queries, torch.Tensor) else type(queries)}")
    return queries.detach().contiguous(), tuple(queries.shape[1:])


def compute_winding_torch(points, normals, area, q, tile=0, differentiable=False):
    """Drop-in for `compute_winding_torch` of examples/eiqonal/single_instance/02_differentiable_winding_number.py:15-30, with its
    shapes and quirks: points, normals (B, Np, 3), area (B, Np, 1), q (1, 3, n, n, n);
        out[0, b, j, i, k] = sum_p area_p ((x_p - q_ijk) . n_p) / |x_p - q_ijk|_1^3,    q_ijk = q[0, :, i, j, k]
    -- no constant in front, the L1 distance cubed, result (1, B, n, n, n) with the first two grid axes swapped.  The reference's
    loop bounds only work for cubic grids and a q of batch 1; anything else is rejected.  One launch instead of n^2 broadcast
    reductions.  differentiable=False (the default): inputs are used detached and nothing is recorded (the reference's scripts only
    threshold the result).  differentiable=True: the result carries the gradient with respect to points, normals and area (fused
    backward pass, once differentiable); a q that requires grad is a ValueError that names winding_field_composed."""
    if not isinstance(q, torch.Tensor) or q.dim() != 5 or q.shape[1] != 3:
        raise ValueError(f"q must be a tensor (1, 3, n, n, n), got {tuple(q.shape) if isinstance(q, torch.Tensor) else type(q)}")
    if q.shape[0] != 1:
        raise ValueError(f"q must have batch 1 (the reference broadcasts one probe grid over all clouds), got batch {q.shape[0]}")
    n = q.shape[2]
    if q.shape[3] != n or q.shape[4] != n:
        raise ValueError(f"q must be a cubic grid (the reference's loop bounds mix the axes), got {tuple(q.shape[2:])}")
    if not isinstance(area, torch.Tensor):
        raise ValueError("area must be a tensor (B, Np, 1)")
    pts, nrm, ar = _cloud(points, normals, area, detach=not differentiable)
    if pts.shape[-1] != 3:
        raise ValueError(f"points must be (B, Np, 3), got {tuple(points.shape)}")
    if differentiable:
        w = winding_field_ad(pts, nrm, ar, q[0].contiguous(), "l1", 3, 1.0, tile=tile)
    else:
        w, _ = ops.winding_field(pts, nrm, ar, q.detach()[0].contiguous(), metric="l1", power=3, scale=1.0, tile=tile)
    return w.reshape(1, pts.shape[0], n, n, n).transpose(2, 3)


def winding_number(points, normals, area, queries, tile=0, differentiable=False):
    """The generalised winding number of an oriented point cloud on the nodes of a grid:
        w[b, q] = 1 / (2 pi) sum_p area_p ((x_p - q) . n_p) / |x_p - q|^2      (2-D)
        w[b, q] = 1 / (4 pi) sum_p area_p ((x_p - q) . n_p) / |x_p - q|^3      (3-D)
    about 1 inside a closed surface and about 0 outside.  points, normals (B, Np, dim); area (B, Np), (B, Np, 1) or None (= 1);
    queries = stack((xx, yy[, zz])) of a mesh, (dim, Ny, Nx) or (dim, Nz, Ny, Nx).  Returns (B, 1, Ny, Nx) or (B, 1, Nz, Ny, Nx), the
    mesh's own order.  differentiable=False (the default): inputs are used detached, nothing is recorded.  differentiable=True: the
    result carries the gradient with respect to points, normals and area (fused backward pass, once differentiable); queries that
    require grad are a ValueError that names winding_field_composed."""
    pts, nrm, ar = _cloud(points, normals, area, detach=not differentiable)
    dim = pts.shape[-1]
    if differentiable:
        _no_query_grad(queries)
    qs, grid = _grid_queries(queries, dim)
    scale = 1.0 / (2.0 * (dim - 1) * math.pi)
    if differentiable:
        w = winding_field_ad(pts, nrm, ar, qs, "l2", dim, scale, tile=tile)
    else:
        w, _ = ops.winding_field(pts, nrm, ar, qs, metric="l2", power=dim, scale=scale, tile=tile)
    return w.reshape(pts.shape[0], 1, *grid)


def winding_mask(points, normals, area, queries, threshold=0.5, metric="l2", dtype=torch.uint8, tile=0):
    """The inside mask `winding > threshold` in mesh order, (B, 1, Ny, Nx) or (B, 1, Nz, Ny, Nx), compared in the kernel: the field
    is never stored.  metric "l2": the true winding number (see winding_number); "l1": the reference's form (L1 distance to the
    power dim, no constant).  dtype uint8 is ready as a Dirichlet mask of the fused operators, float32 as a network input.
    Not differentiable."""
    if dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"dtype must be torch.uint8 or torch.float32, got {dtype}")
    if metric not in ("l1", "l2"):
        raise ValueError(f"metric must be 'l1' or 'l2', got {metric!r}")
    pts, nrm, ar = _cloud(points, normals, area)
    dim = pts.shape[-1]
    qs, grid = _grid_queries(queries, dim)
    scale = 1.0 / (2.0 * (dim - 1) * math.pi) if metric == "l2" else 1.0
    _, m = ops.winding_field(pts, nrm, ar, qs, metric=metric, power=dim, scale=scale, threshold=threshold, want_field=False, want_mask=True,
                             tile=tile)
    m = m.reshape(pts.shape[0], 1, *grid)
    return m if dtype == torch.uint8 else m.to(dtype)


def read_xyzna(path):
    """The reference's .xyzna text format (examples/eiqonal/single_instance/xyzna_reader.py): a line with the count N, then N lines
    `x y z`, N lines `nx ny nz` and N lines with one area each.  Returns float64 arrays (N, 3), (N, 3), (N, 1)."""
    with open(path) as fh:
        n = int(fh.readline().strip())
        rows = [fh.readline().split() for _ in range(3 * n)]
    if n < 1 or any(len(r) < 3 for r in rows[:2 * n]) or any(len(r) < 1 for r in rows[2 * n:]):
        raise ValueError(f"{path}: not an xyzna file of {n} points (short or missing lines)")
    pts = np.array([[float(v) for v in r[:3]] for r in rows[:n]])
    nrm = np.array([[float(v) for v in r[:3]] for r in rows[n:2 * n]])
    area = np.array([[float(r[0])] for r in rows[2 * n:]])
    return pts, nrm, area
