"""2-D scalar transport residuals with SUPG stabilisation on the HIP operators -- the weak forms of three residual-minimisation scripts of
the reference under `examples/poisson/single_instance/`: `e17_adv_diff_2d_resmin.py:99-171` (AdvDiff2d.loss, steady advection-diffusion),
`e3_st_mms_resmin.py:97-173` (SpaceTimeHeat.loss_resmin, space-time heat with y as time) and `e18_allen_cahn_ice_melt.py:77-151`
(AllenCahnIceMelt.loss, space-time Allen-Cahn with a cubic reaction).

    u~ = where(bc2, value2, where(bc1, value1, u));  at every Gauss point, from u~ and nu (a nodal field evaluated there; None: 1):
    adv = ax u_x + ay u_y                      r(u) = c0 + c1 u + c2 u^2 + c3 u^3
    A = adv + r(u) - f      B = kx nu u_x + tau ax (adv - f)      C = ky nu u_y + tau ay (adv - f)
    R = assemble(sum_g wscale w_g (N_a A + Nx_a B + Ny_a C)),  then the Dirichlet rows of R take the condition's VALUE
    loss = sum R^2

Where both masks are set, condition 2 wins on u; on R condition 2 wins too (e17, e18) unless `r_first_wins` (e3).  The coefficient helpers
return the scripts' (adv, kappa, tau, react); `wscale` defaults to (hx/2)(hy/2).

`transport_residual` / `transport_loss` are ONE fused launch forward (dn_transport_apply, csrc/transport.hip) and one backward: the VJP
launch of the same kernel.  The operator is not symmetric (advection) and the reaction is nonlinear, so the backward is a hand-derived
pullback in the same flux form: with the cotangent evaluated like a field (L, L_x, L_y) and q = L + tau (ax L_x + ay L_y),
A' = L r'(u), B' = ax q + kx nu L_x, C' = ay q + ky nu L_y.  `transport_residual_composed` is the same computation spelled with the
single-launch HIP operators (`gauss_pt_evaluation*`, `assemble`) and torch elementwise ops, differentiable by autograd with respect to
every tensor input; the fused functions are differentiable with respect to u only, so when `nu`, `f_gp` or a value field requires a
gradient the public functions take the composed route (no input gets a silent zero gradient)."""
import math

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .stokes import _fix, _forcing, _weak_form


def advdiff_coefficients(fem, adv, diffusivity):
    """(adv, kappa, tau, react) of e17_adv_diff_2d_resmin.py: tau = 1 / (2 |adv| / h + 4 D / h^2)."""
    ax, ay = float(adv[0]), float(adv[1])
    h, D = float(fem.h), float(diffusivity)
    return (ax, ay), (D, D), 1.0 / (2.0 * math.hypot(ax, ay) / h + 4.0 * D / h ** 2), (0.0, 0.0, 0.0, 0.0)


def space_time_heat_coefficients(fem, diffusivity):
    """(adv, kappa, tau, react) of e3_st_mms_resmin.py: y is time, diffusion along x only, tau = h / 2."""
    return (0.0, 1.0), (float(diffusivity), 0.0), 0.5 * float(fem.h), (0.0, 0.0, 0.0, 0.0)


def allen_cahn_coefficients(A, Cn, D, k):
    """(adv, kappa, tau, react) of e18_allen_cahn_ice_melt.py: D G(u) = D (2 D A (u - 3 u^2 + 2 u^3) - D k), no stabilisation."""
    A, Cn, D, k = float(A), float(Cn), float(D), float(k)
    return (0.0, 1.0), (D * Cn ** 2, D * Cn ** 2), 0.0, (-D * D * k, 2.0 * D * D * A, -6.0 * D * D * A, 4.0 * D * D * A)


def _vals2(bc_values):
    vals = tuple(bc_values)
    if len(vals) != 2:
        raise ValueError("bc_values must hold two entries (condition 1, condition 2)")
    return vals


def _coef(fem, adv, kappa, tau, react, wscale, r_first_wins):
    ws = (0.5 * fem.hx) * (0.5 * fem.hy) if wscale is None else float(wscale)
    return dict(adv=tuple(float(x) for x in adv), kappa=tuple(float(x) for x in kappa), tau=float(tau), react=tuple(float(x) for x in react),
                wscale=ws, r_first_wins=bool(r_first_wins))


def _needs_composed(nu, f_gp, vals):
    return any(isinstance(t, torch.Tensor) and t.requires_grad for t in (nu, f_gp, *vals))


class _TransportResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, fem, nu, bc, bc_values, f_gp, coef):
        out, _ = ops.transport_apply(fem.geom, u, nu, bc, bc_values, f_gp=f_gp, want_sums=False, **coef)
        ctx.save_for_backward(u)
        ctx.fem, ctx.args = fem, (nu, bc, bc_values, f_gp, coef)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        nu, bc, bc_values, f_gp, coef = ctx.args
        out, _ = ops.transport_apply(ctx.fem.geom, ctx.saved_tensors[0], nu, bc, bc_values, f_gp=f_gp, cot=g.contiguous(), want_sums=False, **coef)
        return out, None, None, None, None, None, None


class _TransportLoss(torch.autograd.Function):
    """sum R^2 (or ||R||) written by the launch that computes the residual (in-kernel fixed-order fp64 sum); its VJP is ONE VJP launch on
    the saved residual, which the kernel scales by 2 gout (gout / ||R||) as it loads it."""

    @staticmethod
    def forward(ctx, u, fem, nu, bc, bc_values, f_gp, coef, norm):
        if norm:
            out, _, val = ops.transport_apply(fem.geom, u, nu, bc, bc_values, f_gp=f_gp, want_sums=False, want_norm=True, **coef)
        else:
            out, val = ops.transport_apply(fem.geom, u, nu, bc, bc_values, f_gp=f_gp, **coef)
            val = val.float()
        ctx.save_for_backward(u, out, val)
        ctx.fem, ctx.args, ctx.norm = fem, (nu, bc, bc_values, f_gp, coef), norm
        return val[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        u, R, val = ctx.saved_tensors
        nu, bc, bc_values, f_gp, coef = ctx.args
        g = gout.reshape(1).float()
        kw = dict(in_num=g.contiguous(), in_den=val) if ctx.norm else dict(in_num=2.0 * g)
        out, _ = ops.transport_apply(ctx.fem.geom, u, nu, bc, bc_values, f_gp=f_gp, cot=R, want_sums=False, **coef, **kw)
        return out, None, None, None, None, None, None, None


def transport_residual(fem, u, bc=None, bc_values=(0.0, 0.0), nu=None, f_gp=None, adv=(0.0, 0.0), kappa=(1.0, 1.0), tau=0.0,
                       react=(0.0, 0.0, 0.0, 0.0), wscale=None, r_first_wins=False):
    """Assembled residual R of the transport weak form; one fused launch, differentiable wrt u (one VJP launch)."""
    vals = _vals2(bc_values)
    if _needs_composed(nu, f_gp, vals):
        return transport_residual_composed(fem, u, bc, vals, nu, f_gp, adv, kappa, tau, react, wscale, r_first_wins)
    return _TransportResidual.apply(u, fem, nu, bc, vals, f_gp, _coef(fem, adv, kappa, tau, react, wscale, r_first_wins))


def transport_loss(fem, u, bc=None, bc_values=(0.0, 0.0), nu=None, f_gp=None, adv=(0.0, 0.0), kappa=(1.0, 1.0), tau=0.0,
                   react=(0.0, 0.0, 0.0, 0.0), wscale=None, r_first_wins=False, kind="sumsq"):
    """The scripts' loss sum R^2 (`kind="norm"`: the Frobenius norm ||R||) as one differentiable scalar; one launch forward, one backward."""
    if kind not in ("sumsq", "norm"):
        raise ValueError(f"kind must be 'sumsq' or 'norm', got {kind!r}")
    vals = _vals2(bc_values)
    if _needs_composed(nu, f_gp, vals):
        R = transport_residual_composed(fem, u, bc, vals, nu, f_gp, adv, kappa, tau, react, wscale, r_first_wins)
        return torch.norm(R) if kind == "norm" else torch.sum(R ** 2)
    return _TransportLoss.apply(u, fem, nu, bc, vals, f_gp, _coef(fem, adv, kappa, tau, react, wscale, r_first_wins), kind == "norm")


_CONST = {}


def _const(dev, value):
    """The cotangent scale of *_loss_and_grad (d sum R^2 / dR = 2 R; gout = 1 of the norm): one cached (1,) tensor per device and value"""
    key = (dev.type, dev.index, value)
    t = _CONST.get(key)
    if t is None:
        t = _CONST[key] = torch.full((1,), value, dtype=torch.float32, device=dev)
    return t


def transport_loss_and_grad(fem, u, bc=None, bc_values=(0.0, 0.0), nu=None, f_gp=None, adv=(0.0, 0.0), kappa=(1.0, 1.0), tau=0.0,
                            react=(0.0, 0.0, 0.0, 0.0), wscale=None, r_first_wins=False, kind="sumsq"):
    """(loss, grad): sum R^2 as a float64 0-dim tensor (`kind="norm"`: ||R||, float32) and its gradient with respect to u -- what
    `transport_loss(...).backward()` leaves in u.grad -- from two launches and no autograd graph."""
    if kind not in ("sumsq", "norm"):
        raise ValueError(f"kind must be 'sumsq' or 'norm', got {kind!r}")
    coef, vals = _coef(fem, adv, kappa, tau, react, wscale, r_first_wins), _vals2(bc_values)
    with torch.no_grad():
        if kind == "norm":
            R, _, val = ops.transport_apply(fem.geom, u, nu, bc, vals, f_gp=f_gp, want_sums=False, want_norm=True, **coef)
            grad, _ = ops.transport_apply(fem.geom, u, nu, bc, vals, f_gp=f_gp, cot=R, want_sums=False, in_num=_const(u.device, 1.0), in_den=val,
                                          **coef)
        else:
            R, val = ops.transport_apply(fem.geom, u, nu, bc, vals, f_gp=f_gp, **coef)
            grad, _ = ops.transport_apply(fem.geom, u, nu, bc, vals, f_gp=f_gp, cot=R, want_sums=False, in_num=_const(u.device, 2.0), **coef)
    return val[0], grad


def transport_residual_composed(fem, u, bc=None, bc_values=(0.0, 0.0), nu=None, f_gp=None, adv=(0.0, 0.0), kappa=(1.0, 1.0), tau=0.0,
                                react=(0.0, 0.0, 0.0, 0.0), wscale=None, r_first_wins=False):
    """Same residual from the single-launch HIP operators (3-4 gauss_pt_eval launches + torch elementwise + one assembly), batched and
    differentiable by autograd with respect to u, nu, f_gp and the value fields."""
    c = _coef(fem, adv, kappa, tau, react, wscale, r_first_wins)
    (ax, ay), (kx, ky), tau, (c0, c1, c2, c3) = c["adv"], c["kappa"], c["tau"], c["react"]
    m1, m2 = ops.transport_bc2(bc)
    v1, v2 = _vals2(bc_values)
    u = _fix(_fix(u, m1, v1), m2, v2)
    ev, dx, dy = fem.gauss_pt_evaluation, fem.gauss_pt_evaluation_der_x, fem.gauss_pt_evaluation_der_y
    ux, uy = dx(u), dy(u)
    f = _forcing(0.0 if f_gp is None else f_gp, ux, fem.geom).expand_as(ux)
    s = ax * ux + ay * uy - f
    A = s + c0
    if c1 != 0.0 or c2 != 0.0 or c3 != 0.0:
        ug = ev(u)
        A = A + ug * (c1 + ug * (c2 + ug * c3))
    if nu is None:
        dfx, dfy = kx * ux, ky * uy
    else:
        nug = ev(nu if nu.dim() == 4 else nu.reshape(-1, 1, *fem.geom.node_shape))
        dfx, dfy = kx * nug * ux, ky * nug * uy
    R = fem.assemble(_weak_form(fem, u.device, c["wscale"])(dfx + (tau * ax) * s, dfy + (tau * ay) * s, A))
    if c["r_first_wins"]:
        return _fix(_fix(R, m2, v2), m1, v1)
    return _fix(_fix(R, m1, v1), m2, v2)
