"""2-D Navier-Stokes residuals with variational-multiscale (VMS) stabilisation on the HIP operators -- the nonlinear stage of the
reference's Navier-Stokes scripts: `examples/navier-stokes/single_instance/e1_ns_ldc_resmin.py:147-313` (calc_tau, calc_residuals, loss),
`e2_ns_fps_resmin.py:293` calc_residuals_ns (the default `eq_type='ns'`), `e2_ns_fps_af_bcmask.py:299`, `e2_ns_fps_af_pc.py:341`,
`b1_stokes_ns_resmin_base.py`, `e4_stokes_ns_cases.py`.

    u~ = where(bc1, u_bc, u), v~ = where(bc2, v_bc, v), p~ = where(bc3, p_bc, p);  at every Gauss point, from u~, v~, p~:
    a1 = u u_x + v u_y, a2 = u v_x + v v_y, d = u_x + v_y, r1 = a1 + p_x - f1, r2 = a2 + p_y - f2
    tau_m = 1 / sqrt(Gx u^2 + Gy v^2 + cinv visco^2 (Gx^2 + Gy^2)), tau_c = sqrt(...) / (gx^2 + gy^2)   (detached, as in the scripts)
    T1_a = N a1 + visco (Nx u_x + Ny u_y) - Nx p - N f1 + tau_m (u Nx + v Ny) r1 - tau_m N (r1 u_x + r2 u_y) - tau_m^2 r1 (r1 Nx + r2 Ny)
           + tau_c Nx d      (T2_a likewise with v, Ny, f2)
    T3_a = N d + tau_m (Nx r1 + Ny r2)
    R_k = where(bc_k, value_k, assemble(sum_g wscale w_g T_k))        (Dirichlet rows take the boundary VALUE, as in the scripts)

Coefficients of the scripts (defaults here): visco = 1/Re, wscale = (hx/2)(hy/2), tau_h = (hx, hy) the mesh spacing, cinv = 36.  Masks,
values and forcing take the forms of diffnet_amd.stokes (fp32 / bool / uint8 masks, shared or per sample, one for all three fields or
three; value fields or constants; forcing None, a constant or a Gauss-point tensor (B | 1, G, nely, nelx) -- the scripts' fx_gp, fy_gp).
Any batch B >= 1 (the scripts' body broadcasts correctly at B = 1 only).

`ns_residuals` / `ns_loss` / `ns_total_loss` are ONE fused launch forward (dn_ns_apply, csrc/navier_stokes.hip) and one backward: the
VJP launch of the same kernel at the saved point, which pulls the cotangents back through the pointwise derivative of the weak forms with
tau held fixed (the only way it differs from plain autograd, which the scripts also see since they detach tau).  `ns_residuals_composed`
is the same computation spelled with the single-launch HIP operators (`gauss_pt_evaluation*`, `assemble`) and torch elementwise ops,
differentiable by autograd, kept as a second implementation for cross-checks."""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import ops
from .stokes import _fix, _forcing, _ones3, _vals, _weak_form


def _coef(fem, wscale, tau_h, visco, cinv):
    ws = (0.5 * fem.hx) * (0.5 * fem.hy) if wscale is None else float(wscale)
    th = (float(fem.hx), float(fem.hy)) if tau_h is None else tuple(float(x) for x in tau_h)
    if len(th) != 2:
        raise ValueError("tau_h must hold two entries (hx, hy)")
    return dict(visco=float(visco), wscale=ws, tau_h=th, cinv=float(cinv))


class _NsResiduals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v, p, fem, bc, bc_values, f_gp, coef):
        outs, _ = ops.ns_apply(fem.geom, u, v, p, bc, bc_values, f_gp=f_gp, want_sums=False, **coef)
        ctx.save_for_backward(u, v, p)
        ctx.fem, ctx.args = fem, (bc, bc_values, f_gp, coef)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, g1, g2, g3):
        bc, bc_values, f_gp, coef = ctx.args
        gs = [g.contiguous() for g in (g1, g2, g3)]
        outs, _ = ops.ns_apply(ctx.fem.geom, *ctx.saved_tensors, bc, bc_values, f_gp=f_gp, cot=gs, want_sums=False, **coef)
        return outs[0], outs[1], outs[2], None, None, None, None, None


def ns_residuals(fem, u, v, p, bc, bc_values=(0.0, 0.0, 0.0), visco=1.0, f_gp=None, wscale=None, tau_h=None, cinv=36.0):
    """Assembled residuals (R1, R2, R3) of the Navier-Stokes (VMS) weak form; one fused launch, differentiable wrt u, v, p (tau
    detached).  `wscale` defaults to (hx/2)(hy/2), `tau_h` to (hx, hy)."""
    return _NsResiduals.apply(u, v, p, fem, bc, _vals(bc_values), f_gp, _coef(fem, wscale, tau_h, visco, cinv))


class _NsNorms(torch.autograd.Function):
    """The three Frobenius norms (one (3,) tensor) written by the launch that computes the residuals (in-kernel fixed-order fp64 sums); the
    VJP of all three is ONE VJP launch on the saved residuals, which the kernel scales by gout_k / ||R_k|| as it loads them.  `total`: their
    sum as a scalar."""

    @staticmethod
    def forward(ctx, u, v, p, fem, bc, bc_values, f_gp, coef, total):
        outs, _, norms = ops.ns_apply(fem.geom, u, v, p, bc, bc_values, f_gp=f_gp, want_sums=False, want_norms=True, **coef)
        ctx.save_for_backward(u, v, p, *outs, norms)
        ctx.fem, ctx.args, ctx.total = fem, (bc, bc_values, f_gp, coef), total
        return norms.sum() if total else norms

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        u, v, p, r1, r2, r3, norms = ctx.saved_tensors
        bc, bc_values, f_gp, coef = ctx.args
        # d||R_k||/dR_k = R_k / ||R_k||, zero where ||R_k|| == 0 (torch's norm_backward convention); the kernel forms gout[k] / norms[k]
        g = gout.expand(3).contiguous() if ctx.total else gout.contiguous()
        outs, _ = ops.ns_apply(ctx.fem.geom, u, v, p, bc, bc_values, f_gp=f_gp, cot=(r1, r2, r3), want_sums=False, in_num=g, in_den=norms,
                               **coef)
        return outs[0], outs[1], outs[2], None, None, None, None, None, None


def ns_loss(fem, u, v, p, bc, bc_values=(0.0, 0.0, 0.0), visco=1.0, f_gp=None, wscale=None, tau_h=None, cinv=36.0):
    """(||R1||, ||R2||, ||R3||): the three losses of the scripts (one per optimizer, `optimizer_idx`), each differentiable; one launch
    forward, one launch backward for all three cotangents."""
    norms = _NsNorms.apply(u, v, p, fem, bc, _vals(bc_values), f_gp, _coef(fem, wscale, tau_h, visco, cinv), False)
    return norms.unbind(0)


def ns_total_loss(fem, u, v, p, bc, bc_values=(0.0, 0.0, 0.0), visco=1.0, f_gp=None, wscale=None, tau_h=None, cinv=36.0):
    """||R1|| + ||R2|| + ||R3|| as one differentiable scalar (one autograd node)."""
    return _NsNorms.apply(u, v, p, fem, bc, _vals(bc_values), f_gp, _coef(fem, wscale, tau_h, visco, cinv), True)


def ns_loss_and_grad(fem, u, v, p, bc, bc_values=(0.0, 0.0, 0.0), visco=1.0, f_gp=None, wscale=None, tau_h=None, cinv=36.0, weights=None):
    """(norms, grads): the three residual norms as one (3,) tensor and the gradient of sum_k weights[k] * ||R_k|| (weights: a (3,) float32
    device tensor, default ones) with respect to (u, v, p) -- what `ns_total_loss(...).backward()` leaves in the fields' .grad -- from two
    launches and no autograd graph."""
    coef, vals = _coef(fem, wscale, tau_h, visco, cinv), _vals(bc_values)
    with torch.no_grad():
        Rs, _, norms = ops.ns_apply(fem.geom, u, v, p, bc, vals, f_gp=f_gp, want_sums=False, want_norms=True, **coef)
        if weights is None:
            weights = _ones3(u.device)
        grads, _ = ops.ns_apply(fem.geom, u, v, p, bc, vals, f_gp=f_gp, cot=Rs, want_sums=False, in_num=weights, in_den=norms, **coef)
    return norms, grads


def ns_residuals_composed(fem, u, v, p, bc, bc_values=(0.0, 0.0, 0.0), visco=1.0, f_gp=None, wscale=None, tau_h=None, cinv=36.0):
    """Same residuals from the single-launch HIP operators (9 gauss_pt_eval launches + torch elementwise + 3 assemblies), batched and
    differentiable by autograd with tau detached."""
    c = _coef(fem, wscale, tau_h, visco, cinv)
    visco, wscale, (hx, hy), cinv = c["visco"], c["wscale"], c["tau_h"], c["cinv"]
    bc3, vals, f2 = ops.stokes_bc3(bc), _vals(bc_values), ops.stokes_f2(f_gp)
    u, v, p = (_fix(t, m, val) for t, m, val in zip((u, v, p), bc3, vals))
    ev, dx, dy = fem.gauss_pt_evaluation, fem.gauss_pt_evaluation_der_x, fem.gauss_pt_evaluation_der_y
    ug, vg, pg = ev(u), ev(v), ev(p)
    ux, uy, vx, vy, px, py = dx(u), dy(u), dx(v), dy(v), dx(p), dy(p)
    f1, f2 = _forcing(f2[0], pg, fem.geom).expand_as(pg), _forcing(f2[1], pg, fem.geom).expand_as(pg)
    a1, a2, d = ug * ux + vg * uy, ug * vx + vg * vy, ux + vy
    r1, r2 = a1 + px - f1, a2 + py - f2
    # calc_tau of the scripts (float32 g and G), on detached values
    Gx, Gy = float(np.float32(4.0 / hx ** 2)), float(np.float32(4.0 / hy ** 2))
    gx, gy = np.float32(2.0 / hx), np.float32(2.0 / hy)
    diff = float(np.float32(cinv * visco ** 2) * (np.float32(Gx) ** 2 + np.float32(Gy) ** 2))
    temp = torch.sqrt(Gx * ug.detach() ** 2 + Gy * vg.detach() ** 2 + diff)
    tm, tc = 1.0 / temp, temp * float(np.float32(1.0) / (gx * gx + gy * gy))
    tm2 = tm * tm
    weak = _weak_form(fem, u.device, wscale)
    # the test-function coefficients of T1..T3 (N, Nx, Ny terms of the scripts' temp1..temp3)
    R1 = fem.assemble(weak(visco * ux - pg + tm * ug * r1 - tm2 * r1 * r1 + tc * d, visco * uy + tm * vg * r1 - tm2 * r1 * r2,
                           a1 - f1 - tm * (r1 * ux + r2 * uy)))
    R2 = fem.assemble(weak(visco * vx + tm * ug * r2 - tm2 * r2 * r1, visco * vy - pg + tm * vg * r2 - tm2 * r2 * r2 + tc * d,
                           a2 - f2 - tm * (r1 * vx + r2 * vy)))
    R3 = fem.assemble(weak(tm * r1, tm * r2, d))
    return tuple(_fix(R, m, val) for R, m, val in zip((R1, R2, R3), bc3, vals))
