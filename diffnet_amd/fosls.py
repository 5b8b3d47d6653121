"""2-D first-order-system least-squares loss on the HIP operators -- the loss body of the three-field strong-form script of the
reference, `examples/poisson/single_instance/11_manufactured_strong_form_two_dofs.py:37-71` (Poisson.loss on u and the flux (mx, my)).

    u~ = where(bc2, value2, where(bc1, value1, u));  mx, my are free;  at every Gauss point:
    qx = mx - nu u~_x,   qy = my - nu u~_y,   d = mx_x + my_y + fs f              weights = (wq, wd)
    loss = mean over (batch, elements) of sum_g gpw_g wscale (wq (qx^2 + qy^2) + wd d^2)      (`reduction="sum"`: the sum)

The script takes `torch.mean` of the gpw-weighted sums without a Jacobian, hence `wscale` defaults to 1; its weights and `fs` are 1,
`nu` and `f` are nodal fields interpolated with the basis, its conditions are `> 0.5` with values 1 and 0.  `nu` may also be a
constant; the forcing a nodal field `f`, or `f_gp`: a constant or a field at the Gauss points.

The fields are either three (B,1,ny,nx) tensors `u, mx, my` or, as in the script, one packed (B,3,ny,nx) tensor passed as `u` alone
(`mx` and `my` left None): the packed tensor is read, and its packed gradient written, in place.

`fosls_loss` / `fosls_loss_and_grad` are ONE fused launch (dn_fosls_apply, csrc/fosls.hip) that reads every field once and writes the
sum and the three gradients; the autograd backward only scales the saved gradients.  `fosls_loss_composed` is the same loss spelled
with the single-launch HIP operators (`gauss_pt_evaluation*`: eleven launches) and torch elementwise ops, differentiable by autograd with
respect to every tensor input; the fused functions are differentiable with respect to the fields only, so when `nu`, `f`, `f_gp` or a
value field requires a gradient the public functions take the composed route (no input gets a silent zero gradient)."""

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .stokes import _fix, _forcing
from .transport import _vals2


def _weights2(weights):
    weights = tuple(float(x) for x in weights)
    if len(weights) != 2:
        raise ValueError("weights holds two entries (wq, wd)")
    return weights


def _check(fem, reduction):
    if reduction not in ("mean", "sum"):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    geom = fem.geom
    if any((n - 1) % geom.deg for n in geom.sizes):
        raise ValueError(f"a degree-{geom.deg} mesh needs (n - 1) % {geom.deg} == 0 nodes per axis, got {geom.sizes}")


def _fields(u, mx, my):
    """(packed, tensors): one packed (B,3,ny,nx) tensor, or the three fields"""
    if mx is None and my is None:
        if not isinstance(u, torch.Tensor) or u.dim() != 4 or u.shape[1] != 3:
            raise ValueError(f"a packed field tensor is (B, 3, ny, nx) with channels u, mx, my, got {tuple(getattr(u, 'shape', ()))}")
        return True, (u,)
    if mx is None or my is None:
        raise ValueError("pass u, mx and my, or one packed (B, 3, ny, nx) tensor as u alone")
    return False, (u, mx, my)


def _out_scale(fem, first, reduction):
    return 1.0 / (first.shape[0] * fem.geom.nelem_total) if reduction == "mean" else 1.0


def _needs_composed(nu, f, f_gp, vals):
    return any(isinstance(t, torch.Tensor) and t.requires_grad for t in (nu, f, f_gp, *vals))


def _apply(fem, packed, flds, **kw):
    if packed:
        return ops.fosls_apply(fem.geom, fields=flds[0], **kw)
    return ops.fosls_apply(fem.geom, *flds, **kw)


class _FoslsLoss(torch.autograd.Function):
    """The loss and, where a field asks for it, the gradients from ONE launch; the backward scales the saved gradients by grad_output."""

    @staticmethod
    def forward(ctx, fem, packed, nu, bc, bc_values, f, f_gp, weights, fs, wscale, out_scale, *flds):
        need = tuple(ctx.needs_input_grad[11:])
        ctx.need = need
        want = any(need) if packed else need
        grads, s = _apply(fem, packed, flds, nu=nu, bc=bc, bc_values=bc_values, f=f, f_gp=f_gp, weights=weights, fs=fs, wscale=wscale,
                          out_scale=out_scale, want_grad=want)
        if any(need):
            ctx.save_for_backward(*((grads,) if packed else [g for g in grads if g is not None]))
        return (s[0] * out_scale).float()

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        saved = iter(ctx.saved_tensors)
        return (None,) * 11 + tuple(next(saved) * gout if n else None for n in ctx.need)


def fosls_loss(fem, u, mx=None, my=None, nu=None, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, weights=(1.0, 1.0), fs=1.0, wscale=1.0,
               reduction="mean"):
    """The first-order-system least-squares loss as one differentiable float32 scalar: one fused launch forward, which also leaves the
    gradients with respect to u, mx and my (or the packed tensor) for the backward (no second launch)."""
    _check(fem, reduction)
    vals, weights = _vals2(bc_values), _weights2(weights)
    packed, flds = _fields(u, mx, my)
    if _needs_composed(nu, f, f_gp, vals):
        return fosls_loss_composed(fem, u, mx, my, nu, bc, vals, f, f_gp, weights, fs, wscale, reduction)
    return _FoslsLoss.apply(fem, packed, nu, bc, vals, f, f_gp, weights, float(fs), float(wscale), _out_scale(fem, flds[0], reduction), *flds)


def fosls_loss_and_grad(fem, u, mx=None, my=None, nu=None, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, weights=(1.0, 1.0), fs=1.0,
                        wscale=1.0, reduction="mean"):
    """(loss, grads): the loss as a float64 0-dim tensor and its gradients -- (gu, gmx, gmy), or one packed (B,3,ny,nx) tensor for a
    packed input: what `fosls_loss(...).backward()` leaves in .grad -- from one launch and no autograd graph."""
    _check(fem, reduction)
    vals, weights = _vals2(bc_values), _weights2(weights)
    packed, flds = _fields(u, mx, my)
    scale = _out_scale(fem, flds[0], reduction)
    with torch.no_grad():
        grads, s = _apply(fem, packed, flds, nu=nu, bc=bc, bc_values=vals, f=f, f_gp=f_gp, weights=weights, fs=float(fs),
                          wscale=float(wscale), out_scale=scale)
        return s[0] * scale, grads


def fosls_residuals_composed(fem, u, mx=None, my=None, nu=None, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, fs=1.0):
    """(qx, qy, d) at the Gauss points (B, G, nely, nelx each) from the single-launch HIP operators (the script's eleven Gauss-point
    evaluations, fewer where nu or the forcing is a constant) and torch elementwise ops, differentiable by autograd with respect to
    the fields, nu, f, f_gp and the value fields."""
    packed, flds = _fields(u, mx, my)
    if packed:
        u, mx, my = (flds[0][:, k:k + 1] for k in range(3))
    if f is not None and isinstance(f_gp, torch.Tensor):
        raise ValueError("nodal forcing f and Gauss-point forcing f_gp exclude each other")
    m1, m2 = ops.transport_bc2(bc)
    v1, v2 = _vals2(bc_values)
    u = _fix(_fix(u, m1, v1), m2, v2)
    geom = fem.geom
    ux, uy = fem.gauss_pt_evaluation_der_x(u), fem.gauss_pt_evaluation_der_y(u)
    if isinstance(nu, torch.Tensor) and nu.numel() > 1:
        nug = fem.gauss_pt_evaluation(nu if nu.dim() == 4 else nu.reshape(-1, 1, *geom.node_shape))
    else:
        nug = 1.0 if nu is None else float(nu)
    qx = fem.gauss_pt_evaluation(mx) - nug * ux
    qy = fem.gauss_pt_evaluation(my) - nug * uy
    d = fem.gauss_pt_evaluation_der_x(mx) + fem.gauss_pt_evaluation_der_y(my)
    if float(fs) != 0.0:
        if f is not None:
            fg = fem.gauss_pt_evaluation(f if f.dim() == 4 else f.reshape(-1, 1, *geom.node_shape))
        else:
            fg = _forcing(0.0 if f_gp is None else f_gp, d, geom)
        d = d + float(fs) * fg
    return qx, qy, d


def fosls_loss_composed(fem, u, mx=None, my=None, nu=None, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, weights=(1.0, 1.0), fs=1.0,
                        wscale=1.0, reduction="mean"):
    """Same loss on the composed route, batched and differentiable by autograd with respect to every tensor input."""
    _check(fem, reduction)
    wq, wd = _weights2(weights)
    qx, qy, d = fosls_residuals_composed(fem, u, mx, my, nu, bc, bc_values, f, f_gp, fs)
    jac = (fem.gpw.to(d.device) * float(wscale)).reshape(1, -1, 1, 1).type_as(d)
    per_elem = torch.sum(jac * (wq * (qx ** 2 + qy ** 2)), 1) + torch.sum(jac * (wd * d ** 2), 1)
    return torch.mean(per_elem) if reduction == "mean" else torch.sum(per_elem)
