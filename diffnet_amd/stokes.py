"""2-D Stokes residuals with PSPG pressure stabilisation on the HIP operators -- the three-field weak form of the reference's Stokes
scripts: `examples/stokes/single_instance/e2_stokes_ldc_resmin.py:151-240`, `e1_stokes_mms_resmin.py:122-217`,
`e1_stokes_mms_resmin_loss2.py:158-247`, and the Stokes stage of the Navier-Stokes scripts
(`navier-stokes/single_instance/e2_ns_fps_resmin.py:193` calc_residuals_stokes, `e2_ns_fps_af_bcmask.py:199`,
`e2_ns_fps_af_pc.py:234`, `b1_stokes_ns_resmin_base.py:181`).

    u~ = where(bc1, u_bc, u), v~ = where(bc2, v_bc, v), p~ = where(bc3, p_bc, p)
    R1_a = sum_e sum_g J w_g [ visco (Nx_a u~_x + Ny_a u~_y) - Nx_a p~ - N_a f1 ]
    R2_a = sum_e sum_g J w_g [ visco (Nx_a v~_x + Ny_a v~_y) - Ny_a p~ - N_a f2 ]
    R3_a = sum_e sum_g J w_g [ N_a (u~_x + v~_y) + pspg (Nx_a p~_x + Ny_a p~_y) ]
    R_k = where(bc_k, value_k, R_k)        (Dirichlet rows take the boundary VALUE, as in the scripts)

Coefficients of the scripts (h: element size, Re: Reynolds number):
  - e2_stokes_ldc_resmin, e1_stokes_mms_resmin_loss2: visco = 1/Re, pspg = h^2 Re / 12, wscale = (h/2)^2;
  - e1_stokes_mms_resmin: visco = Re (that script multiplies the viscous term by Re), pspg = h^2 Re / 12, wscale = (h/2)^2;
  - the Navier-Stokes scripts' Stokes stage: visco = 1/Re, pspg = hx hy Re / 12, wscale = 1 (`trnsfrm_jac = 1.`), no forcing.

Masks: fp32 (`>= 0.5`, the scripts' test) or bool / uint8 (non-zero), shared by the batch or per sample; `bc` is one mask for the three
fields or three (None: no condition).  Forcing `f_gp = (f1, f2)`: each None, a constant or a Gauss-point tensor (G, nely, nelx) /
(B | 1, G, nely, nelx) -- the scripts' `fx_gp`, `fy_gp`.  Any batch B >= 1 (the scripts' body broadcasts correctly at B = 1 only).

`stokes_residuals` / `stokes_loss` / `stokes_total_loss` are ONE fused launch forward (dn_stokes_apply, csrc/stokes.hip) and one backward:
the Jacobian is J_R = P A P with A's coupling blocks -C (momentum) and C^T (continuity), so J_R^T = S J_R S with S = diag(1, 1, -1) and the
VJP is the same kernel in its transpose mode.  `stokes_residuals_composed` is the same computation spelled with the single-launch HIP
operators (`gauss_pt_evaluation*`, `assemble`) and torch elementwise ops, kept as a second implementation for cross-checks."""
import torch
from torch.autograd.function import once_differentiable

from . import ops


def _wscale(fem, wscale):
    return (0.5 * fem.hx) * (0.5 * fem.hy) if wscale is None else float(wscale)


def _vals(bc_values):
    vals = tuple(bc_values)
    if len(vals) != 3:
        raise ValueError("bc_values must hold three entries (u, v, p)")
    return vals


class _StokesResiduals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v, p, fem, bc, bc_values, visco, pspg, f_gp, wscale):
        outs, _ = ops.stokes_apply(fem.geom, u, v, p, bc, bc_values, visco, pspg, f_gp, wscale, want_sums=False)
        ctx.fem, ctx.bc, ctx.coef = fem, bc, (visco, pspg, wscale)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, g1, g2, g3):
        visco, pspg, wscale = ctx.coef
        gs = [g.contiguous() for g in (g1, g2, g3)]
        outs, _ = ops.stokes_apply(ctx.fem.geom, *gs, ctx.bc, (0.0, 0.0, 0.0), visco, pspg, None, wscale, want_sums=False, transpose=True)
        return outs[0], outs[1], outs[2], None, None, None, None, None, None, None


def stokes_residuals(fem, u, v, p, bc, bc_values=(0.0, 0.0, 0.0), visco=1.0, pspg=0.0, f_gp=None, wscale=None):
    """Assembled residuals (R1, R2, R3) of the Stokes (PSPG) weak form; one fused launch, differentiable wrt u, v, p.  `wscale` defaults to
    (hx/2)(hy/2)."""
    return _StokesResiduals.apply(u, v, p, fem, bc, _vals(bc_values), visco, pspg, f_gp, _wscale(fem, wscale))


class _StokesLoss(torch.autograd.Function):
    """The three Frobenius norms (one (3,) tensor) written by the launch that computes the residuals (in-kernel fixed-order fp64 sums); the
    VJP of all three is ONE transpose launch on the saved residuals, which the kernel scales by gout_k / ||R_k|| as it loads them.  `total`:
    their sum as a scalar."""

    @staticmethod
    def forward(ctx, u, v, p, fem, bc, bc_values, visco, pspg, f_gp, wscale, total):
        outs, _, norms = ops.stokes_apply(fem.geom, u, v, p, bc, bc_values, visco, pspg, f_gp, wscale, want_sums=False, want_norms=True)
        ctx.save_for_backward(*outs, norms)
        ctx.fem, ctx.bc, ctx.coef, ctx.total = fem, bc, (visco, pspg, wscale), total
        return norms.sum() if total else norms

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        *Rs, norms = ctx.saved_tensors
        visco, pspg, wscale = ctx.coef
        # d||R_k||/dR_k = R_k / ||R_k||, zero where ||R_k|| == 0 (torch's norm_backward convention); the kernel forms gout[k] / norms[k]
        g = gout.expand(3).contiguous() if ctx.total else gout.contiguous()
        outs, _ = ops.stokes_apply(ctx.fem.geom, *Rs, ctx.bc, (0.0, 0.0, 0.0), visco, pspg, None, wscale, want_sums=False,
                                   in_num=g, in_den=norms, transpose=True)
        return outs[0], outs[1], outs[2], None, None, None, None, None, None, None, None


def stokes_loss(fem, u, v, p, bc, bc_values=(0.0, 0.0, 0.0), visco=1.0, pspg=0.0, f_gp=None, wscale=None):
    """(||R1||, ||R2||, ||R3||): the three losses of the scripts (one per optimizer, `optimizer_idx`), each differentiable; one launch
    forward, one launch backward for all three cotangents."""
    norms = _StokesLoss.apply(u, v, p, fem, bc, _vals(bc_values), visco, pspg, f_gp, _wscale(fem, wscale), False)
    return norms.unbind(0)


def stokes_total_loss(fem, u, v, p, bc, bc_values=(0.0, 0.0, 0.0), visco=1.0, pspg=0.0, f_gp=None, wscale=None):
    """||R1|| + ||R2|| + ||R3|| as one differentiable scalar (the loss of e1_stokes_mms_resmin.py:214-217)."""
    return _StokesLoss.apply(u, v, p, fem, bc, _vals(bc_values), visco, pspg, f_gp, _wscale(fem, wscale), True)


_ONES = {}


def _ones3(dev):
    """The default weights of *_loss_and_grad: one cached (3,) vector of ones per device."""
    key = (dev.type, dev.index)
    ones = _ONES.get(key)
    if ones is None:
        ones = _ONES[key] = torch.ones(3, dtype=torch.float32, device=dev)
    return ones


def stokes_loss_and_grad(fem, u, v, p, bc, bc_values=(0.0, 0.0, 0.0), visco=1.0, pspg=0.0, f_gp=None, wscale=None, weights=None):
    """(norms, grads): the three residual norms as one (3,) tensor and the gradient of sum_k weights[k] * ||R_k|| (weights: a (3,) float32
    device tensor, default ones) with respect to (u, v, p) -- what `stokes_total_loss(...).backward()` leaves in the fields' .grad -- from two
    launches and no autograd graph."""
    wscale = _wscale(fem, wscale)
    with torch.no_grad():
        Rs, _, norms = ops.stokes_apply(fem.geom, u, v, p, bc, _vals(bc_values), visco, pspg, f_gp, wscale, want_sums=False, want_norms=True)
        if weights is None:
            weights = _ones3(u.device)
        grads, _ = ops.stokes_apply(fem.geom, *Rs, bc, (0.0, 0.0, 0.0), visco, pspg, None, wscale, want_sums=False, in_num=weights,
                                    in_den=norms, transpose=True)
    return norms, grads


def _condition(m):
    if m.dtype == torch.bool:
        return m
    if m.dtype == torch.uint8:
        return m != 0
    return m >= 0.5


# ---- the composed route (shared with navier_stokes.ns_residuals_composed) ----

def _fix(t, m, val):
    """where(m, val, t): the Dirichlet substitution of a field / the Dirichlet rows of a residual"""
    if m is None:
        return t
    return torch.where(_condition(m), val if isinstance(val, torch.Tensor) else torch.full_like(t, float(val)), t)


def _forcing(f, pg, geom):
    """A forcing term (constant or Gauss-point tensor) at the Gauss points, shaped like the Gauss-point field pg (B | 1 samples)"""
    if isinstance(f, torch.Tensor) and f.numel() > 1:
        return f.to(pg.device).reshape(-1, geom.ngp_total, *geom.elem_shape)
    return torch.full_like(pg, float(f))


def _weak_form(fem, dev, wscale):
    """weak(a_x, a_y, a_0) = sum_g JxW ( dN_x a_x + dN_y a_y + N a_0 ), per local basis function -> (B, nbf, nelY, nelX)"""
    N, Nx, Ny = (t.to(dev) for t in (fem.Nvalues, fem.dN_x_values, fem.dN_y_values))       # (1, nbf, ngp, 1, 1)
    jxw = (fem.gpw.to(dev) * wscale).reshape(1, 1, -1, 1, 1)

    def weak(a_x, a_y, a_0):
        t = Nx * a_x.unsqueeze(1) + Ny * a_y.unsqueeze(1) + N * a_0.unsqueeze(1)
        return torch.sum(t * jxw, 2)

    return weak


def stokes_residuals_composed(fem, u, v, p, bc, bc_values=(0.0, 0.0, 0.0), visco=1.0, pspg=0.0, f_gp=None, wscale=None):
    """Same residuals from the single-launch HIP operators (9 gauss_pt_eval launches + torch elementwise + 3 assemblies), batched."""
    wscale = _wscale(fem, wscale)
    bc3, vals, f2 = ops.stokes_bc3(bc), _vals(bc_values), ops.stokes_f2(f_gp)
    u, v, p = (_fix(t, m, val) for t, m, val in zip((u, v, p), bc3, vals))
    ev, dx, dy = fem.gauss_pt_evaluation, fem.gauss_pt_evaluation_der_x, fem.gauss_pt_evaluation_der_y
    ux, uy, vx, vy = dx(u), dy(u), dx(v), dy(v)
    pg, px, py = ev(p), dx(p), dy(p)
    weak = _weak_form(fem, u.device, wscale)
    R1 = fem.assemble(weak(visco * ux - pg, visco * uy, -_forcing(f2[0], pg, fem.geom).expand_as(pg)))
    R2 = fem.assemble(weak(visco * vx, visco * vy - pg, -_forcing(f2[1], pg, fem.geom).expand_as(pg)))
    R3 = fem.assemble(weak(pspg * px, pspg * py, ux + vy))
    return tuple(_fix(R, m, val) for R, m, val in zip((R1, R2, R3), bc3, vals))
