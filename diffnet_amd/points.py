"""Point-cloud terms on a structured mesh: evaluate a nodal field and its gradient at points, the scripts' penalty loss and its gradient
-- what every point-cloud script of the reference adds to a loss this library already fuses (`examples/poisson/single_instance/
pc_poisson_disk.py`, `pc_complex_immersed_background.py`; `examples/eiqonal/parametric/10_fixed_bc.py`, `single_instance/
02_2d_curve_recon.py`, `e01_curve_reconstruction.py`, `04_3d_sphere_recon.py`, `05_3d_sphere_loss4.py`; `e2_ns_fps_af_pc.py`).

    u_p = sum_a N_a(xi_p) u_a          g_d = s_d sum_a d_d N_a(xi_p) u_a        over the nodes a of the point's element
    loss = w_val sum_p (u_p - t_p)^2 + w_nrm sum_p (g . n - 1)^2                 kind "dot"    (10_fixed_bc.py:208, 05_3d_sphere_loss4.py:389)
                                     + w_nrm sum_p sum_d (g_d - n_d)^2           kind "match"  (e01_curve_reconstruction.py:270)

`s_d` (`dscale`) is 1 for the scripts' reference-coordinate derivative (`bf_1d_der_th`) or 2 / h_d ("physical") for the gradient in
domain coordinates.  A mean is a weight.

All data-dependent addressing is settled once, in a `PointPlan` built with torch ops: every point is classified into its element,
clamped, given local coordinates and sorted by (sample, element).  On a Q1 mesh and a GPU tensor, `eval_at_points`, `point_loss` and
`point_loss_and_grad` are then ONE launch forward (dn_points_apply, csrc/point_terms.hip: one thread per point) and one backward (a
dense gather over the nodes: no atomics, bitwise reproducible -- where the autograd backward of the torch form ends in an index_put
with accumulation).  `point_terms_composed` is the same arithmetic in plain torch (gather, weights, sums): the route for CPU tensors,
other dtypes, Q2 / Q3 meshes and fields other than u that need a gradient.
"""
import torch
from torch.autograd.function import once_differentiable

from . import ops

KINDS = ("none", "dot", "match")


def _geom(fem):
    return getattr(fem, "geom", fem)


class PointPlan:
    """Classification of a point cloud against the mesh of `fem` (a DiffNetFEM, or its FemGeometry), built with torch ops only.

    points: (B, P, nsd), or (P, nsd) shared by `batch` samples, in domain coordinates, on the device the terms will run on.
    Per axis, the element index is e_d = trunc(x_d / h_d) evaluated in the points' own dtype, as the scripts write it
    (`(pc[..., d] / self.hx).long()`), then clamped to [0, nel_d - 1]: a point on the far face x = L belongs to the last element with
    xi = +1 (the scripts read one node past the array there).  `classify="float64"` divides the up-cast points instead.  Points outside
    [0, L] on any axis (L = h_d nel_d, to its rounding) and non-finite points raise ValueError (`validate=False` skips the check and its
    one host synchronisation: points are then clamped into the nearest element and extrapolated).  The local coordinate
    xi_d = 2 (x_d - e_d h_d) / h_d - 1 is computed in float64 and rounded once to float32.

    axes: which tensor axis each point column indexes.  None: the physical order -- x the last axis, y the one before it, z the first
    spatial axis (05_3d_sphere_loss4.py:345).  "transposed": column c indexes spatial axis c, the 2-D scripts' `u[b, 0, nidx, nidy]`
    where x indexes rows.  Or a tuple of spatial axes, one per column.  A column is measured with the spacing of the axis it indexes;
    per-point results (gradients, normals, dscale) stay in the caller's column order.

    The plan holds, sorted by (sample, flat element id) with a stable sort: `elem` (T = B P, int32), `xi` (nsd, T) float32 in the
    kernels' axis order (last tensor axis first), the permutation `order` (sorted position -> original flat index), its inverse
    `inv`, and `offsets` (B nel + 1, int32), the CSR of the sorted list (searchsorted: no host synchronisation).  Build it once for a
    fixed cloud; for a cloud that changes every step the build is a handful of torch launches (two elementwise passes per axis, one
    sort, two gathers, one searchsorted)."""

    def __init__(self, fem, points, axes=None, classify="reference", batch=None, validate=True):
        geom = _geom(fem)
        self.geom, nsd = geom, geom.nsd
        if not isinstance(points, torch.Tensor) or not points.is_floating_point():
            raise TypeError("PointPlan: points must be a floating-point tensor")
        if points.dim() == 2:
            points = points[None].expand(1 if batch is None else int(batch), *points.shape)
        elif batch is not None and points.shape[0] != batch:
            raise ValueError(f"PointPlan: points hold {points.shape[0]} samples, batch is {batch}")
        if points.dim() != 3 or points.shape[2] != nsd:
            raise ValueError(f"PointPlan: points must be (B, P, {nsd}) or (P, {nsd}), got {tuple(points.shape)}")
        if classify not in ("reference", "float64"):
            raise ValueError(f"PointPlan: classify must be 'reference' or 'float64', got {classify!r}")
        if axes is None:
            axes = tuple(nsd - 1 - c for c in range(nsd))
        elif isinstance(axes, str):
            if axes != "transposed":
                raise ValueError(f"PointPlan: axes must be None, 'transposed' or a tuple of spatial axes, got {axes!r}")
            axes = tuple(range(nsd))
        axes = tuple(int(a) for a in axes)
        if sorted(axes) != list(range(nsd)):
            raise ValueError(f"PointPlan: axes must be a permutation of {tuple(range(nsd))}, got {axes}")
        self.axes = axes
        # kernel axis k (0: the last tensor axis, the mesh's x) is fed by point column cols[k]
        self.cols = tuple(axes.index(nsd - 1 - k) for k in range(nsd))
        self.B, self.P = int(points.shape[0]), int(points.shape[1])
        self.T, self.device = self.B * self.P, points.device
        nel, hs = geom.nel, geom.hs
        nel_total = geom.nelem_total

        p64 = points.double()
        if validate and self.T:
            hi = torch.empty(nsd, dtype=torch.float64)
            for k in range(nsd):
                hi[self.cols[k]] = hs[k] * nel[k] * (1.0 + 2.0 ** -50)
            hi = hi.to(points.device)
            bad = ~(torch.isfinite(p64) & (p64 >= 0.0) & (p64 <= hi))
            if bool(bad.any()):
                b, p, c = (int(v) for v in bad.nonzero()[0])
                raise ValueError(f"PointPlan: point {p} of sample {b} has coordinate {float(points[b, p, c])!r} in column {c}, outside [0, {float(hi[c]):.9g}]")
        flat = torch.zeros((self.B, self.P), dtype=torch.int64, device=points.device)
        xi, stride = [], 1
        for k in range(nsd):
            x, h = points[..., self.cols[k]], hs[k]
            e = ((x / h) if classify == "reference" else (p64[..., self.cols[k]] / h)).long().clamp(0, nel[k] - 1)
            xi.append((2.0 * (p64[..., self.cols[k]] - e.double() * h) / h - 1.0).float().reshape(-1))
            flat += e * stride
            stride *= nel[k]
        key = (flat + torch.arange(self.B, device=points.device)[:, None] * nel_total).reshape(-1)
        skey, order = torch.sort(key, stable=True)
        self.order = order
        self.inv = torch.empty_like(order)
        self.inv[order] = torch.arange(self.T, device=points.device)
        self.elem = (skey % nel_total).to(torch.int32)
        self.xi = torch.stack(xi)[:, order].contiguous()
        self.offsets = torch.searchsorted(skey, torch.arange(self.B * nel_total + 1, device=points.device)).to(torch.int32)
        self._sorted = []

    # -- the caller's per-point tensors in the plan's order and back ---------------------------------------------------------------
    def sort(self, t, vector=False):
        """A per-point tensor in the caller's order -- (B, P) / (P,), or with `vector` (B, P, nsd) / (P, nsd) in the caller's column
        order -- in the sorted order of the plan: (T), or (nsd, T) in the kernels' axis order.  One gather; the result for a tensor
        that has not changed since (the same tensor object at the same version; the plan keeps the last few alive, so that no other
        tensor can take their place in memory) is kept: a fixed cloud's normals are sorted once."""
        src = t
        for kept, version, vec, out in self._sorted:
            if kept is t and version == t._version and vec == vector:
                return out
        want = (self.B, self.P, self.geom.nsd) if vector else (self.B, self.P)
        if tuple(t.shape) == want[1:]:
            t = t[None].expand(want)
        if tuple(t.shape) != want:
            raise ValueError(f"PointPlan: a per-point tensor must be {want} or {want[1:]}, got {tuple(t.shape)}")
        if vector:
            out = t.reshape(self.T, self.geom.nsd)[self.order][:, list(self.cols)].t().contiguous()
        else:
            out = t.reshape(self.T)[self.order]
        if not src.requires_grad:
            self._sorted = self._sorted[-7:] + [(src, src._version, vector, out)]
        return out

    def unsort(self, v, vector=False):
        """The inverse of `sort`: (T) -> (B, P), (nsd, T) in kernel axis order -> (B, P, nsd) in the caller's column order."""
        if vector:
            back = [self.cols.index(c) for c in range(self.geom.nsd)]           # caller's column c is kernel axis back[c]
            return v[back][:, self.inv].t().reshape(self.B, self.P, self.geom.nsd)
        return v[self.inv].reshape(self.B, self.P)

    def dscale(self, dscale):
        """`dscale` -- None / 1 (reference-coordinate derivative), "physical" (2 / h of the axis a column indexes), a float, or one value
        per point column -- as the kernels' three floats (x, y, z)."""
        nsd, hs = self.geom.nsd, self.geom.hs
        if dscale is None:
            return (1.0,) * nsd
        if isinstance(dscale, str):
            if dscale != "physical":
                raise ValueError(f"dscale must be None, 'physical', a float or one float per column, got {dscale!r}")
            return tuple(2.0 / hs[k] for k in range(nsd))
        if isinstance(dscale, (int, float)):
            return (float(dscale),) * nsd
        if len(dscale) != nsd:
            raise ValueError(f"dscale holds {len(dscale)} values for {nsd} columns")
        return tuple(float(dscale[self.cols[k]]) for k in range(nsd))


def _basis(xi, deg):
    """Values and derivatives (deg + 1, T) of the 1-D Lagrange basis on equispaced nodes of [-1, 1] at xi (T)."""
    if deg == 1:
        half = torch.full_like(xi, 0.5)
        return torch.stack((0.5 * (1.0 - xi), 0.5 * (1.0 + xi))), torch.stack((-half, half))
    nodes = [-1.0 + 2.0 * a / deg for a in range(deg + 1)]
    val, der = [], []
    for a in range(deg + 1):
        den = 1.0
        for m in range(deg + 1):
            if m != a:
                den *= nodes[a] - nodes[m]
        v, d = torch.ones_like(xi), torch.zeros_like(xi)
        for m in range(deg + 1):
            if m == a:
                continue
            t = torch.ones_like(xi)
            for q in range(deg + 1):
                if q != a and q != m:
                    t = t * (xi - nodes[q])
            d = d + t
            v = v * (xi - nodes[m])
        val.append(v / den)
        der.append(d / den)
    return torch.stack(val), torch.stack(der)


def _composed_eval(geom, u, plan, ds):
    """(values (T), grads (nsd, T)) in the plan's order, plain torch: gather the (deg + 1)^nsd nodes of each point's element, weight, sum."""
    nsd, deg, B = geom.nsd, geom.deg, plan.B
    if tuple(u.shape) != (B, 1, *geom.node_shape):
        raise ValueError(f"field shape {tuple(u.shape)} != {(B, 1, *geom.node_shape)}")
    e = plan.elem.long()
    idx = torch.arange(B, device=u.device).repeat_interleave(plan.P) * geom.nnode_total          # (T) -> (nodes of the element, T)
    idx = idx[None]
    W = torch.ones((1, plan.T), dtype=u.dtype, device=u.device)
    D = [W] * nsd                                                                                   # d_j N: the derivative on axis j, values on the others
    stride, n = 1, 1
    for k in range(nsd):
        n *= deg + 1
        ek = e % geom.nel[k]
        e = e // geom.nel[k]
        val, der = _basis(plan.xi[k].to(u.dtype), deg)                                              # (nb, T)
        node = (ek[None] * deg + torch.arange(deg + 1, device=u.device)[:, None]) * stride          # (nb, T)
        idx = (node[:, None] + idx[None]).reshape(n, plan.T)                                        # axis k varies slowest
        W = (val[:, None] * W[None]).reshape(n, plan.T)
        D = [((der if j == k else val)[:, None] * D[j][None]).reshape(n, plan.T) for j in range(nsd)]
        stride *= geom.sizes[k]
    up = u.reshape(-1)[idx]
    vals = (up * W).sum(0)
    grads = torch.stack([ds[k] * (up * D[k]).sum(0) for k in range(nsd)])
    return vals, grads


def _penalty(vals, grads, target, normals, kind, w_val, w_nrm):
    lv = w_val * torch.sum((vals - target) ** 2)
    if kind == "none":
        return lv, torch.zeros_like(lv)
    if kind == "dot":
        return lv, w_nrm * torch.sum(((grads * normals).sum(0) - 1.0) ** 2)
    return lv, w_nrm * torch.sum((grads - normals) ** 2)


def _check(kind, normals):
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    if normals is None:
        return "none"
    return kind


def _sorted_inputs(plan, u, target, normals, kind):
    tgt = plan.sort(target.to(u.dtype)) if isinstance(target, torch.Tensor) and target.numel() > 1 else float(target)
    nrm = plan.sort(normals.to(u.dtype), vector=True) if kind != "none" else None
    return tgt, nrm


def point_terms_composed(fem, u, plan, target=0.0, normals=None, kind="dot", w_val=1.0, w_nrm=1.0, dscale=None, terms=False):
    """The penalty loss in plain torch ops, any device, dtype and element degree, differentiable by autograd with respect to u, target
    and normals; `terms`: (value term, normals term) instead of their sum."""
    geom = _geom(fem)
    kind = _check(kind, normals)
    tgt, nrm = _sorted_inputs(plan, u, target, normals, kind)
    vals, grads = _composed_eval(geom, u, plan, plan.dscale(dscale))
    lv, ln = _penalty(vals, grads, tgt, nrm, kind, w_val, w_nrm)
    return (lv, ln) if terms else lv + ln


def eval_at_points_composed(fem, u, plan, dscale=None):
    """`eval_at_points` in plain torch ops."""
    vals, grads = _composed_eval(_geom(fem), u, plan, plan.dscale(dscale))
    return plan.unsort(vals), plan.unsort(grads, vector=True)


def _fused(geom, u, *others):
    """The fused launches serve float32 GPU fields on Q1 meshes, and differentiate with respect to u only."""
    return geom.deg == 1 and u.is_cuda and u.dtype == torch.float32 and not any(isinstance(t, torch.Tensor) and t.requires_grad for t in others)


class _EvalAtPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, geom, plan, ds):
        vals, grads, _, _, _ = ops.points_apply(geom, plan.B, plan.P, plan.xi, plan.elem, u=u.contiguous(), dscale=ds, want_values=True, want_pgrads=True)
        ctx.geom, ctx.plan, ctx.ds = geom, plan, ds
        return plan.unsort(vals), plan.unsort(grads, vector=True)

    @staticmethod
    @once_differentiable
    def backward(ctx, gv, gg):
        plan = ctx.plan
        cot = torch.cat((plan.sort(gv.contiguous())[None], plan.sort(gg.contiguous(), vector=True)))
        grad = ops.points_apply(ctx.geom, plan.B, plan.P, plan.xi, offsets=plan.offsets, dscale=ctx.ds, cot=cot, want_grad=True)[4]
        return grad, None, None, None


class _PointLoss(torch.autograd.Function):
    """The penalty written by the launch that evaluates the points (in-kernel fixed-order fp64 sums), with the per-point cotangents; its
    backward is the adjoint launch on them, scaled by the upstream gradient in the kernel."""

    @staticmethod
    def forward(ctx, u, geom, plan, kw):
        _, _, sums, cot, _ = ops.points_apply(geom, plan.B, plan.P, plan.xi, plan.elem, u=u.contiguous(), penalty=True, want_sums=True, want_cot=True, **kw)
        ctx.save_for_backward(cot)
        ctx.geom, ctx.plan, ctx.ds = geom, plan, kw["dscale"]
        return sums[2].float()

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        plan = ctx.plan
        grad = ops.points_apply(ctx.geom, plan.B, plan.P, plan.xi, offsets=plan.offsets, dscale=ctx.ds, cot=ctx.saved_tensors[0], want_grad=True,
                                gscale_dev=gout.reshape(1).float().contiguous())[4]
        return grad, None, None, None


def _kw(plan, u, target, normals, kind, w_val, w_nrm, dscale):
    tgt, nrm = _sorted_inputs(plan, u, target, normals, kind)
    return dict(dscale=plan.dscale(dscale), kind=kind, target=tgt, normals=nrm, w_val=float(w_val), w_nrm=float(w_nrm))


def eval_at_points(fem, u, plan, dscale=None):
    """(values (B, P), grads (B, P, nsd)) of the field u (B,1,*node_shape) at the plan's points, in the caller's original point and
    column order; differentiable with respect to u.  One launch forward, one backward on a float32 GPU field of a Q1 mesh; the composed
    torch route otherwise."""
    geom = _geom(fem)
    if not _fused(geom, u):
        return eval_at_points_composed(fem, u, plan, dscale)
    return _EvalAtPoints.apply(u, geom, plan, plan.dscale(dscale))


def point_loss(fem, u, plan, target=0.0, normals=None, kind="dot", w_val=1.0, w_nrm=1.0, dscale=None):
    """w_val sum_p (u_p - target_p)^2 + w_nrm (the normals term of `kind`; none without normals) as one differentiable float32 scalar.
    target: a float or a (B, P) / (P,) tensor; normals: (B, P, nsd) / (P, nsd) in the caller's column order.  One launch forward and one
    backward (the adjoint, with the upstream gradient as its scale) on a float32 GPU field of a Q1 mesh; the composed torch route for
    CPU tensors, other dtypes, Q2 / Q3 meshes, or when target or normals need a gradient."""
    geom = _geom(fem)
    kind = _check(kind, normals)
    if not _fused(geom, u, target, normals):
        return point_terms_composed(fem, u, plan, target, normals, kind, w_val, w_nrm, dscale)
    return _PointLoss.apply(u, geom, plan, _kw(plan, u, target, normals, kind, w_val, w_nrm, dscale))


def point_loss_and_grad(fem, u, plan, target=0.0, normals=None, kind="dot", w_val=1.0, w_nrm=1.0, dscale=None, grad_out=None, accumulate=False,
                        gscale=1.0):
    """(loss, grad) outside autograd, from two launches issued by one call: the loss as a float64 0-dim tensor and gscale times its
    gradient with respect to u -- into a fresh tensor, into `grad_out`, or with `accumulate` added to `grad_out` (the buffer another
    loss_and_grad has just written)."""
    geom = _geom(fem)
    kind = _check(kind, normals)
    if accumulate and grad_out is None:
        raise ValueError("point_loss_and_grad: accumulate adds to grad_out")
    with torch.no_grad():
        if _fused(geom, u):
            _, _, sums, _, grad = ops.points_apply(geom, plan.B, plan.P, plan.xi, plan.elem, plan.offsets, u=u.contiguous(), penalty=True, want_sums=True,
                                                   want_grad=True, grad_out=grad_out, accumulate=accumulate, gscale=gscale,
                                                   **_kw(plan, u, target, normals, kind, w_val, w_nrm, dscale))
            return sums[2], grad
    v = u.detach().requires_grad_(True)
    loss = point_terms_composed(fem, v, plan, target, normals, kind, w_val, w_nrm, dscale)
    g, = torch.autograd.grad(loss, v)
    g = g * gscale
    if grad_out is None:
        return loss.detach().double(), g
    with torch.no_grad():
        grad_out.add_(g) if accumulate else grad_out.copy_(g)
    return loss.detach().double(), grad_out
