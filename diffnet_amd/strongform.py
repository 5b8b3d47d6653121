"""2-D strong-form least-squares losses on the HIP operators -- the loss bodies of the two reference scripts that call the
second-derivative Gauss-point evaluations: `examples/burgers/single_instance/01_2d_space_time.py:73-96` (Burgers.loss, space-time
Burgers on Q2 with y as time) and `examples/poisson/single_instance/10_manufactured_strong_form_higher_order.py:69-96` (Poisson.loss,
strong-form Poisson on Q3).

    u~ = where(bc2, value2, where(bc1, value1, u));  at every Gauss point, from u~:
    r = ax u_x + ay u_y + b u u_x + dxx u_xx + dyy u_yy + fs f                    coef = (ax, ay, b, dxx, dyy, fs)
    loss = mean over (batch, elements) of sum_g gpw_g wscale r_g^2                (`reduction="sum"`: the sum)

The scripts take `torch.mean` of the gpw-weighted sums without a Jacobian, hence `wscale` defaults to 1.  The forcing is a nodal field
`f` (interpolated with the basis, as script 10 does), or `f_gp`: a constant or a field at the Gauss points.

`strong_form_loss` / `strong_form_loss_and_grad` are ONE fused launch (dn_strongform_apply, csrc/strongform.hip) that reads u once and
writes the sum and its gradient; the autograd backward only scales the saved gradient.  `strong_form_loss_composed` is the same loss
spelled with the single-launch HIP operators (`gauss_pt_evaluation*`, `_der2_x` / `_der2_y` included) and torch elementwise ops,
differentiable by autograd with respect to every tensor input; the fused functions are differentiable with respect to u only, so when
`f`, `f_gp` or a value field requires a gradient the public functions take the composed route (no input gets a silent zero gradient)."""

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .stokes import _fix, _forcing
from .transport import _vals2

_NO_TERMS = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def burgers_coefficients(viscosity=0.0):
    """(ax, ay, b, dxx, dyy, fs) of 01_2d_space_time.py: u_t + u u_x with y as time; `viscosity` nu adds -nu u_xx (the script evaluates
    u_xx but leaves it out of its loss; its dataset's nu is 0.01 / pi)."""
    return (0.0, 1.0, 1.0, -float(viscosity), 0.0, 0.0)


def poisson_strong_coefficients():
    """(ax, ay, b, dxx, dyy, fs) of 10_manufactured_strong_form_higher_order.py: u_xx + u_yy + f."""
    return (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)


def _coef6(coef):
    coef = tuple(float(x) for x in coef)
    if len(coef) != 6:
        raise ValueError("coef holds six entries (ax, ay, b, dxx, dyy, fs)")
    return coef


def _check(fem, reduction):
    if reduction not in ("mean", "sum"):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    geom = fem.geom
    if any((n - 1) % geom.deg for n in geom.sizes):
        raise ValueError(f"a degree-{geom.deg} mesh needs (n - 1) % {geom.deg} == 0 nodes per axis, got {geom.sizes}")


def _out_scale(fem, u, reduction):
    return 1.0 / (u.shape[0] * fem.geom.nelem_total) if reduction == "mean" else 1.0


def _needs_composed(f, f_gp, vals):
    return any(isinstance(t, torch.Tensor) and t.requires_grad for t in (f, f_gp, *vals))


class _StrongFormLoss(torch.autograd.Function):
    """The loss and, where u asks for it, its gradient from ONE launch; the backward scales the saved gradient by grad_output."""

    @staticmethod
    def forward(ctx, u, fem, bc, bc_values, f, f_gp, coef, wscale, out_scale):
        want_grad = ctx.needs_input_grad[0]
        grad, s = ops.strongform_apply(fem.geom, u, bc, bc_values, f, f_gp, coef, wscale, out_scale, want_grad=want_grad)
        if want_grad:
            ctx.save_for_backward(grad)
        return (s[0] * out_scale).float()

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        grad, = ctx.saved_tensors
        return grad * gout, None, None, None, None, None, None, None, None


def strong_form_loss(fem, u, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, coef=_NO_TERMS, wscale=1.0, reduction="mean"):
    """The strong-form least-squares loss as one differentiable float32 scalar: one fused launch forward, which also leaves the
    gradient with respect to u for the backward (no second launch)."""
    _check(fem, reduction)
    vals, coef = _vals2(bc_values), _coef6(coef)
    if _needs_composed(f, f_gp, vals):
        return strong_form_loss_composed(fem, u, bc, vals, f, f_gp, coef, wscale, reduction)
    return _StrongFormLoss.apply(u, fem, bc, vals, f, f_gp, coef, float(wscale), _out_scale(fem, u, reduction))


def strong_form_loss_and_grad(fem, u, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, coef=_NO_TERMS, wscale=1.0, reduction="mean"):
    """(loss, grad): the loss as a float64 0-dim tensor and its gradient with respect to u -- what `strong_form_loss(...).backward()`
    leaves in u.grad -- from one launch and no autograd graph."""
    _check(fem, reduction)
    vals, coef = _vals2(bc_values), _coef6(coef)
    scale = _out_scale(fem, u, reduction)
    with torch.no_grad():
        grad, s = ops.strongform_apply(fem.geom, u, bc, vals, f, f_gp, coef, float(wscale), scale)
        return s[0] * scale, grad


def strong_form_residual_composed(fem, u, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, coef=_NO_TERMS):
    """The residual r at the Gauss points (B, G, nely, nelx) from the single-launch HIP operators (one gauss_pt_eval launch per term
    present) and torch elementwise ops, differentiable by autograd with respect to u, f, f_gp and the value fields."""
    ax, ay, b, dxx, dyy, fs = _coef6(coef)
    if f is not None and isinstance(f_gp, torch.Tensor):
        raise ValueError("nodal forcing f and Gauss-point forcing f_gp exclude each other")
    m1, m2 = ops.transport_bc2(bc)
    v1, v2 = _vals2(bc_values)
    u = _fix(_fix(u, m1, v1), m2, v2)
    geom = fem.geom
    ux = fem.gauss_pt_evaluation_der_x(u) if (ax != 0.0 or b != 0.0) else None
    r = None

    def add(r, t):
        return t if r is None else r + t

    if ax != 0.0:
        r = add(r, ax * ux)
    if ay != 0.0:
        r = add(r, ay * fem.gauss_pt_evaluation_der_y(u))
    if b != 0.0:
        r = add(r, b * fem.gauss_pt_evaluation(u) * ux)
    if dxx != 0.0:                            # (degree 1: the tables are zero, and the result still is a function of u for autograd)
        r = add(r, dxx * fem.gauss_pt_evaluation_der2_x(u))
    if dyy != 0.0:
        r = add(r, dyy * fem.gauss_pt_evaluation_der2_y(u))
    if r is None:
        r = 0.0 * fem.gauss_pt_evaluation(u)
    if fs != 0.0:
        if f is not None:
            fg = fem.gauss_pt_evaluation(f if f.dim() == 4 else f.reshape(-1, 1, *geom.node_shape))
        else:
            fg = _forcing(0.0 if f_gp is None else f_gp, r, geom)
        r = r + fs * fg
    return r


def strong_form_loss_composed(fem, u, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, coef=_NO_TERMS, wscale=1.0, reduction="mean"):
    """Same loss on the composed route, batched and differentiable by autograd with respect to every tensor input."""
    _check(fem, reduction)
    r = strong_form_residual_composed(fem, u, bc, bc_values, f, f_gp, coef)
    jac = (fem.gpw.to(r.device) * float(wscale)).reshape(1, -1, 1, 1).type_as(r)
    per_elem = torch.sum(jac * r ** 2, 1)
    return torch.mean(per_elem) if reduction == "mean" else torch.sum(per_elem)
