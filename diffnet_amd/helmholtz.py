"""2-D Helmholtz energy loss and weak-form residual on the HIP operators -- the loss body the two Helmholtz scripts of the reference
share, `examples/poisson/single_instance/14_helmholtz_mms.py:37-63` and `14_helmholtz_ddelta.py:37-63` (Poisson.loss), on the datasets
`RectangleHelmholtzManufactured` and `RectangleHelmholtzDeltaForce`, each of which carries its `khh`.

    u~ = where(bc2, value2, where(bc1, value1, u));  at every Gauss point, from u~:
    energy density = c nu (u_x^2 + u_y^2) - cr sigma u^2 - fs u f              the scripts: c = cr = 0.5, sigma = khh^2, fs = 1
    loss = mean over (batch, elements) of sum_g gpw_g wscale density_g          (`reduction="sum"`: the sum)
    R_a  = zero_on_dirichlet( sum_e sum_g gpw_g wscale ( nu gradN_a . grad u~ - sigma N_a u~ - N_a f ) )     the weak-form residual

The scripts take `torch.mean` of the gpw-weighted sums without a Jacobian, hence `wscale` defaults to 1.  `nu` is None (1) or a nodal
field, `sigma` a constant or a nodal field, the forcing a nodal field `f` (interpolated with the basis, as the scripts do) or `f_gp`:
a constant or a field at the Gauss points.

The energy is indefinite once sigma exceeds the lowest eigenvalue of the Laplacian (2 pi^2 on the unit square): minimising it is then
not a solve, while minimising sum R^2 stays well posed (what the reference's *_resmin scripts do for Poisson).

`helmholtz_energy_loss` / `helmholtz_energy_loss_and_grad` are ONE fused launch (dn_helmholtz_apply, csrc/helmholtz.hip) that reads u
once and writes the energy and its gradient; the autograd backward only scales the saved gradient.  `helmholtz_residual` is one launch;
`helmholtz_residual_loss` / `helmholtz_residual_loss_and_grad` are two: R with its sum of squares, then -- the operator is symmetric --
the same operator on R without forcing and with zero Dirichlet values for the gradient.  `helmholtz_energy_loss_composed` and
`helmholtz_residual_composed` are the same functions spelled with the single-launch HIP operators (`gauss_pt_evaluation*` and their
adjoints) and torch elementwise ops, differentiable by autograd with respect to every tensor input; the fused functions are
differentiable with respect to u only, so when `nu`, `sigma`, `f`, `f_gp` or a value field requires a gradient the public functions
take the composed route (no input gets a silent zero gradient)."""

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .stokes import _fix, _forcing
from .transport import _vals2


def helmholtz_coefficients(khh):
    """The constants of 14_helmholtz_mms.py / 14_helmholtz_ddelta.py as keyword arguments of the losses here:
    0.5 (nu |grad u|^2 - khh^2 u^2) - u f."""
    return dict(sigma=float(khh) ** 2, c=0.5, cr=0.5, fs=1.0)


def _check(fem, reduction):
    if reduction not in ("mean", "sum"):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    geom = fem.geom
    if any((n - 1) % geom.deg for n in geom.sizes):
        raise ValueError(f"a degree-{geom.deg} mesh needs (n - 1) % {geom.deg} == 0 nodes per axis, got {geom.sizes}")


def _energy_scale(fem, u, reduction):
    return 1.0 / (u.shape[0] * fem.geom.nelem_total) if reduction == "mean" else 1.0


def _residual_scale(fem, u, reduction):
    return 1.0 / (u.shape[0] * fem.geom.nnode_total) if reduction == "mean" else 1.0


def _needs_composed(nu, sigma, f, f_gp, vals):
    return any(isinstance(t, torch.Tensor) and t.requires_grad for t in (nu, sigma, f, f_gp, *vals))


class _EnergyLoss(torch.autograd.Function):
    """The loss and, where u asks for it, its gradient from ONE launch; the backward scales the saved gradient by grad_output."""

    @staticmethod
    def forward(ctx, u, fem, nu, sigma, bc, bc_values, f, f_gp, coef, wscale, out_scale):
        want_out = ctx.needs_input_grad[0]
        c, cr, fs = coef
        out, e, _ = ops.helmholtz_apply(fem.geom, u, nu, sigma, bc, bc_values, f, f_gp, coef, (2.0 * c, 2.0 * cr, fs), wscale, out_scale,
                                        want_out=want_out)
        if want_out:
            ctx.save_for_backward(out)
        return (e[0] * out_scale).float()

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        out, = ctx.saved_tensors
        return (out * gout,) + (None,) * 10


def helmholtz_energy_loss(fem, u, nu=None, sigma=0.0, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, c=0.5, cr=0.5, fs=1.0, wscale=1.0,
                          reduction="mean"):
    """The Helmholtz energy as one differentiable float32 scalar: one fused launch forward, which also leaves the gradient with respect
    to u for the backward (no second launch)."""
    _check(fem, reduction)
    vals = _vals2(bc_values)
    if _needs_composed(nu, sigma, f, f_gp, vals):
        return helmholtz_energy_loss_composed(fem, u, nu, sigma, bc, vals, f, f_gp, c, cr, fs, wscale, reduction)
    return _EnergyLoss.apply(u, fem, nu, sigma, bc, vals, f, f_gp, (float(c), float(cr), float(fs)), float(wscale),
                             _energy_scale(fem, u, reduction))


def helmholtz_energy_loss_and_grad(fem, u, nu=None, sigma=0.0, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, c=0.5, cr=0.5, fs=1.0,
                                   wscale=1.0, reduction="mean"):
    """(loss, grad): the energy as a float64 0-dim tensor and its gradient with respect to u -- what
    `helmholtz_energy_loss(...).backward()` leaves in u.grad -- from one launch and no autograd graph."""
    _check(fem, reduction)
    vals = _vals2(bc_values)
    scale = _energy_scale(fem, u, reduction)
    c, cr, fs = float(c), float(cr), float(fs)
    with torch.no_grad():
        out, e, _ = ops.helmholtz_apply(fem.geom, u, nu, sigma, bc, vals, f, f_gp, (c, cr, fs), (2.0 * c, 2.0 * cr, fs), float(wscale), scale)
        return e[0] * scale, out


def _transposed(fem, v, nu, sigma, bc, wscale, out_scale=1.0):
    """The operator on v without forcing and with zero Dirichlet values: by symmetry, the transposed Jacobian of the residual on v."""
    out, _, _ = ops.helmholtz_apply(fem.geom, v, nu, sigma, bc, (0.0, 0.0), None, None, (0.0, 0.0, 0.0), (1.0, 1.0, 0.0), wscale, out_scale,
                                    want_energy=False)
    return out


class _Residual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, fem, nu, sigma, bc, bc_values, f, f_gp, wscale):
        out, _, _ = ops.helmholtz_apply(fem.geom, u, nu, sigma, bc, bc_values, f, f_gp, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), wscale, 1.0,
                                        want_energy=False)
        ctx.fem, ctx.args = fem, (nu, sigma, bc, wscale)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        return (_transposed(ctx.fem, gout.contiguous(), *ctx.args),) + (None,) * 8


def helmholtz_residual(fem, u, nu=None, sigma=0.0, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, wscale=1.0):
    """The assembled weak-form residual R (B,1,ny,nx), zero on the Dirichlet nodes: one launch; its backward is one more."""
    _check(fem, "sum")
    vals = _vals2(bc_values)
    if _needs_composed(nu, sigma, f, f_gp, vals):
        return helmholtz_residual_composed(fem, u, nu, sigma, bc, vals, f, f_gp, wscale)
    return _Residual.apply(u, fem, nu, sigma, bc, vals, f, f_gp, float(wscale))


class _ResidualLoss(torch.autograd.Function):
    """sum R^2 from the launch that forms R; the backward is the second launch, on R (scaled by 2 * scale through out_scale)."""

    @staticmethod
    def forward(ctx, u, fem, nu, sigma, bc, bc_values, f, f_gp, wscale, scale):
        want_out = ctx.needs_input_grad[0]
        out, _, ss = ops.helmholtz_apply(fem.geom, u, nu, sigma, bc, bc_values, f, f_gp, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), wscale, 1.0,
                                         want_out=want_out, want_energy=False, want_sumsq=True)
        if want_out:
            ctx.save_for_backward(out)
        ctx.fem, ctx.args = fem, (nu, sigma, bc, wscale, 2.0 * scale)
        return (ss[0] * scale).float()

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        out, = ctx.saved_tensors
        return (_transposed(ctx.fem, out, *ctx.args) * gout,) + (None,) * 9


def helmholtz_residual_loss(fem, u, nu=None, sigma=0.0, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, wscale=1.0, reduction="sum"):
    """sum R^2 over batch and nodes (`reduction="mean"`: divided by their number) as one differentiable float32 scalar: one launch
    forward, one more in the backward."""
    _check(fem, reduction)
    vals = _vals2(bc_values)
    if _needs_composed(nu, sigma, f, f_gp, vals):
        r = helmholtz_residual_composed(fem, u, nu, sigma, bc, vals, f, f_gp, wscale)
        return torch.sum(r ** 2) * _residual_scale(fem, u, reduction)
    return _ResidualLoss.apply(u, fem, nu, sigma, bc, vals, f, f_gp, float(wscale), _residual_scale(fem, u, reduction))


def helmholtz_residual_loss_and_grad(fem, u, nu=None, sigma=0.0, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, wscale=1.0,
                                     reduction="sum"):
    """(loss, grad): sum R^2 (or its mean) as a float64 0-dim tensor and its gradient with respect to u, from two launches and no
    autograd graph."""
    _check(fem, reduction)
    vals = _vals2(bc_values)
    scale = _residual_scale(fem, u, reduction)
    with torch.no_grad():
        out, _, ss = ops.helmholtz_apply(fem.geom, u, nu, sigma, bc, vals, f, f_gp, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), float(wscale), 1.0,
                                         want_energy=False, want_sumsq=True)
        return ss[0] * scale, _transposed(fem, out, nu, sigma, bc, float(wscale), 2.0 * scale)


def _gauss_point_fields(fem, u, nu, sigma, bc, bc_values, f, f_gp):
    """(u, u_x, u_y, nu, sigma, f) at the Gauss points from the single-launch operators; nu and sigma as floats where they are constants"""
    if f is not None and isinstance(f_gp, torch.Tensor):
        raise ValueError("nodal forcing f and Gauss-point forcing f_gp exclude each other")
    m1, m2 = ops.transport_bc2(bc)
    v1, v2 = _vals2(bc_values)
    u = _fix(_fix(u, m1, v1), m2, v2)
    geom = fem.geom

    def nodal(t):
        return fem.gauss_pt_evaluation(t if t.dim() == 4 else t.reshape(-1, 1, *geom.node_shape))

    ug, ux, uy = fem.gauss_pt_evaluation(u), fem.gauss_pt_evaluation_der_x(u), fem.gauss_pt_evaluation_der_y(u)
    nug = nodal(nu) if isinstance(nu, torch.Tensor) and nu.numel() > 1 else (1.0 if nu is None else float(nu))
    sgg = nodal(sigma) if isinstance(sigma, torch.Tensor) and sigma.numel() > 1 else (0.0 if sigma is None else float(sigma))
    fg = nodal(f) if f is not None else _forcing(0.0 if f_gp is None else f_gp, ug, geom)
    return ug, ux, uy, nug, sgg, fg


def helmholtz_energy_loss_composed(fem, u, nu=None, sigma=0.0, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, c=0.5, cr=0.5, fs=1.0,
                                   wscale=1.0, reduction="mean"):
    """Same loss on the composed route (the scripts' five Gauss-point evaluations, fewer where nu or sigma is a constant), batched and
    differentiable by autograd with respect to every tensor input."""
    _check(fem, reduction)
    ug, ux, uy, nug, sgg, fg = _gauss_point_fields(fem, u, nu, sigma, bc, bc_values, f, f_gp)
    jac = (fem.gpw.to(ug.device) * float(wscale)).reshape(1, -1, 1, 1).type_as(ug)
    dens = float(c) * nug * (ux ** 2 + uy ** 2) - float(cr) * sgg * ug ** 2 - float(fs) * ug * fg
    per_elem = torch.sum(jac * dens, 1)
    return torch.mean(per_elem) if reduction == "mean" else torch.sum(per_elem)


def helmholtz_residual_composed(fem, u, nu=None, sigma=0.0, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=None, wscale=1.0):
    """The weak-form residual from the single-launch operators and their adjoints (R = gpe^T(W nu u_x; Nx) + gpe^T(W nu u_y; Ny)
    - gpe^T(W (sigma u + f); N), zero on the Dirichlet nodes), differentiable by autograd with respect to every tensor input."""
    ug, ux, uy, nug, sgg, fg = _gauss_point_fields(fem, u, nu, sigma, bc, bc_values, f, f_gp)
    geom = fem.geom
    T, _ = ops._geom_tables(geom, u.device)
    nbf = geom.deg + 1
    wg = (fem.gpw.to(ug.device) * float(wscale)).reshape(1, -1, 1, 1).type_as(ug)
    shape = (u.shape[0], 1, *geom.node_shape)

    def adjoint(q, name):
        return ops._GaussPtEvalT.apply(q.expand(u.shape[0], *q.shape[1:]).contiguous(), T[name], shape, 2, nbf, nbf - 1)

    r = adjoint(wg * nug * ux, "dN_x_gp") + adjoint(wg * nug * uy, "dN_y_gp") - adjoint(wg * (sgg * ug + fg), "N_gp")
    m1, m2 = ops.transport_bc2(bc)
    return _fix(_fix(r, m1, 0.0), m2, 0.0)
