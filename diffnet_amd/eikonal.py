"""2-D and 3-D stabilised eikonal weak-form residual on the HIP operators -- the domain term of the eikonal scripts of the reference under
`examples/eiqonal/`: `parametric/10_fixed_bc.py:127-216` (loss_eikonal) and `single_instance/e01_curve_reconstruction.py:452-558` (loss4).

    u~ = where(bc2, value2, where(bc1, value1, u));  at every Gauss point, from u~:
    A = sq (u_x^2 + u_y^2) - f      B = tau u u_x      C = tau u u_y
    R = zero_on_dirichlet(assemble(sum_g wscale w_g (N_a A + Nx_a B + Ny_a C)))
    loss = ||R||_F  (`kind="norm"`, the scripts' loss)   or   sum R^2  (`kind="sumsq"`)

`sq` defaults to 1 + tau and `wscale` to (hx/2)(hy/2), as in the scripts; the right-hand side is the constant `f_gp` (default 1, the
scripts' `N_values * 1.0`), a Gauss-point field `f_gp` or a nodal field `f` interpolated with the basis.  `tau = 0, sq = 1` is the
unstabilised N (|grad u|^2 - 1) of the older scripts.  The scripts add two point-cloud terms to this loss: `diffnet_amd.points.point_loss`
(examples/eikonal_2d.py).

`eikonal_residual` / `eikonal_loss` are ONE fused launch forward (dn_eikonal_apply, csrc/eikonal.hip) and one backward: the VJP launch
of the same kernel.  The residual is nonlinear -- the diffusion coefficient of the stabilisation is the unknown itself --, so the
backward is a hand-derived pullback in the same flux form: with the cotangent (zero on the Dirichlet nodes) evaluated like a field
(L, L_x, L_y),  A' = tau (L_x u_x + L_y u_y),  B' = 2 sq L u_x + tau u L_x,  C' = 2 sq L u_y + tau u L_y  (DESIGN.md section 3.2).
`eikonal_residual_composed` is the same computation spelled with the single-launch HIP operators (`gauss_pt_evaluation*`, `assemble`)
and torch elementwise ops, differentiable by autograd with respect to every tensor input; the fused functions are differentiable with
respect to u only, so when `f`, `f_gp` or a value field requires a gradient the public functions take the composed route (no input gets
a silent zero gradient).

On a `DiffNet3DFEM` the same functions are the domain term of `single_instance/05_3d_sphere_loss4.py:269-425` (loss4; `04_3d_sphere_recon.py`
is tau = 0, sq = 1, f_gp = h): fields are (B,1,nz,ny,nx), the flux gains  D = tau u u_z  on Nz_a (VJP:  A' = tau grad L . grad u,
D' = 2 sq L u_z + tau u L_z),  `wscale` defaults to (hx/2)(hy/2)(hz/2) and the fused launch is dn_eikonal3d_apply
(csrc/eikonal3d.hip), for Q1 meshes; on a 3-D Q2 or Q3 mesh the fused functions raise and `eikonal_residual_composed` is the route."""
import torch
from torch.autograd.function import once_differentiable

from . import ops
from .stokes import _fix, _forcing, _weak_form
from .transport import _const, _vals2


def eikonal_coefficients(tau):
    """The constants of loss_eikonal / loss4 as keyword arguments of the functions here: tau u grad N . grad u + (1 + tau) N |grad u|^2
    (both scripts set tau = 0.25); the right-hand side N * 1 is the default forcing."""
    tau = float(tau)
    return dict(tau=tau, sq=1.0 + tau)


def _coef(fem, tau, sq, wscale):
    tau = float(tau)
    if wscale is not None:
        ws = float(wscale)
    elif fem.nsd == 3:
        ws = (0.5 * fem.hx) * (0.5 * fem.hy) * (0.5 * fem.hz)
    else:
        ws = (0.5 * fem.hx) * (0.5 * fem.hy)
    return dict(tau=tau, sq=1.0 + tau if sq is None else float(sq), wscale=ws)


def _apply(fem):
    """The fused launch of the mesh: dn_eikonal_apply in 2-D, dn_eikonal3d_apply in 3-D (Q1 only there)"""
    if fem.nsd != 3:
        return ops.eikonal_apply
    if fem.geom.deg != 1:
        raise ops.DiffNetHipError(f"the fused 3-D eikonal residual is compiled for Q1 meshes only (degree {fem.geom.deg}): use "
                                  "eikonal_residual_composed, which takes any degree")
    return ops.eikonal3d_apply


def _kind(kind):
    if kind not in ("sumsq", "norm"):
        raise ValueError(f"kind must be 'sumsq' or 'norm', got {kind!r}")
    return kind == "norm"


def _needs_composed(f, f_gp, vals):
    return any(isinstance(t, torch.Tensor) and t.requires_grad for t in (f, f_gp, *vals))


class _EikonalResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, fem, bc, bc_values, f, f_gp, coef):
        out, _, _ = _apply(fem)(fem.geom, u, bc, bc_values, f, f_gp, **coef)
        ctx.save_for_backward(u)
        ctx.fem, ctx.args = fem, (bc, bc_values, coef)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        bc, bc_values, coef = ctx.args
        out, _, _ = _apply(ctx.fem)(ctx.fem.geom, ctx.saved_tensors[0], bc, bc_values, cot=g.contiguous(), **coef)
        return out, None, None, None, None, None, None


class _EikonalLoss(torch.autograd.Function):
    """||R|| (or sum R^2) written by the launch that computes the residual (in-kernel fixed-order fp64 sum); its VJP is ONE VJP launch on
    the saved residual, which the kernel scales by gout / ||R|| (2 gout) as it loads it."""

    @staticmethod
    def forward(ctx, u, fem, bc, bc_values, f, f_gp, coef, norm):
        out, ss, nrm = _apply(fem)(fem.geom, u, bc, bc_values, f, f_gp, want_sumsq=not norm, want_norm=norm, **coef)
        val = nrm if norm else ss.float()
        ctx.save_for_backward(u, out, val)
        ctx.fem, ctx.args, ctx.norm = fem, (bc, bc_values, coef), norm
        return val[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        u, R, val = ctx.saved_tensors
        bc, bc_values, coef = ctx.args
        g = gout.reshape(1).float()
        kw = dict(in_num=g.contiguous(), in_den=val) if ctx.norm else dict(in_num=2.0 * g)
        out, _, _ = _apply(ctx.fem)(ctx.fem.geom, u, bc, bc_values, cot=R, **coef, **kw)
        return out, None, None, None, None, None, None, None


def eikonal_residual(fem, u, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=1.0, tau=0.0, sq=None, wscale=None):
    """Assembled residual R (B,1,ny,nx) of the eikonal weak form, zero on the Dirichlet nodes; one fused launch, differentiable wrt u
    (one VJP launch)."""
    vals = _vals2(bc_values)
    if _needs_composed(f, f_gp, vals):
        return eikonal_residual_composed(fem, u, bc, vals, f, f_gp, tau, sq, wscale)
    return _EikonalResidual.apply(u, fem, bc, vals, f, f_gp, _coef(fem, tau, sq, wscale))


def eikonal_loss(fem, u, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=1.0, tau=0.0, sq=None, wscale=None, kind="norm"):
    """The scripts' domain loss ||R||_F (`kind="sumsq"`: sum R^2) as one differentiable float32 scalar; one launch forward, one backward."""
    norm = _kind(kind)
    vals = _vals2(bc_values)
    if _needs_composed(f, f_gp, vals):
        R = eikonal_residual_composed(fem, u, bc, vals, f, f_gp, tau, sq, wscale)
        return torch.norm(R) if norm else torch.sum(R ** 2)
    return _EikonalLoss.apply(u, fem, bc, vals, f, f_gp, _coef(fem, tau, sq, wscale), norm)


def eikonal_loss_and_grad(fem, u, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=1.0, tau=0.0, sq=None, wscale=None, kind="norm"):
    """(loss, grad): ||R|| as a float32 0-dim tensor (`kind="sumsq"`: sum R^2, float64) and its gradient with respect to u -- what
    `eikonal_loss(...).backward()` leaves in u.grad -- from two launches and no autograd graph."""
    norm = _kind(kind)
    coef, vals = _coef(fem, tau, sq, wscale), _vals2(bc_values)
    apply = _apply(fem)
    with torch.no_grad():
        R, ss, nrm = apply(fem.geom, u, bc, vals, f, f_gp, want_sumsq=not norm, want_norm=norm, **coef)
        if norm:
            grad, _, _ = apply(fem.geom, u, bc, vals, cot=R, in_num=_const(u.device, 1.0), in_den=nrm, **coef)
            return nrm[0], grad
        grad, _, _ = apply(fem.geom, u, bc, vals, cot=R, in_num=_const(u.device, 2.0), **coef)
        return ss[0], grad


def eikonal_residual_composed(fem, u, bc=None, bc_values=(0.0, 0.0), f=None, f_gp=1.0, tau=0.0, sq=None, wscale=None):
    """Same residual from the single-launch HIP operators (3-4 gauss_pt_eval launches + torch elementwise + one assembly), batched and
    differentiable by autograd with respect to u, f, f_gp and the value fields."""
    if f is not None and isinstance(f_gp, torch.Tensor) and f_gp.numel() > 1:
        raise ValueError("nodal forcing f and Gauss-point forcing f_gp exclude each other")
    c = _coef(fem, tau, sq, wscale)
    tau, sq = c["tau"], c["sq"]
    m1, m2 = ops.transport_bc2(bc)
    v1, v2 = _vals2(bc_values)
    u = _fix(_fix(u, m1, v1), m2, v2)
    ug, ux, uy = fem.gauss_pt_evaluation(u), fem.gauss_pt_evaluation_der_x(u), fem.gauss_pt_evaluation_der_y(u)
    if f is not None:
        fg = fem.gauss_pt_evaluation(f if f.dim() == fem.nsd + 2 else f.reshape(-1, 1, *fem.geom.node_shape))
    else:
        fg = _forcing(1.0 if f_gp is None else f_gp, ug, fem.geom)
    if fem.nsd == 3:
        uz = fem.gauss_pt_evaluation_der_z(u)
        A = sq * (ux ** 2 + uy ** 2 + uz ** 2) - fg.expand_as(ux)
        R = fem.assemble(_weak_form3(fem, u.device, c["wscale"])((tau * ug) * ux, (tau * ug) * uy, (tau * ug) * uz, A))
        return _fix(_fix(R, m1, 0.0), m2, 0.0)
    A = sq * (ux ** 2 + uy ** 2) - fg.expand_as(ux)
    R = fem.assemble(_weak_form(fem, u.device, c["wscale"])((tau * ug) * ux, (tau * ug) * uy, A))
    return _fix(_fix(R, m1, 0.0), m2, 0.0)


def _weak_form3(fem, dev, wscale):
    """weak(a_x, a_y, a_z, a_0) = sum_g JxW ( dN_x a_x + dN_y a_y + dN_z a_z + N a_0 ), per local basis function -> (B, nbf, nelZ, nelY, nelX)"""
    N, Nx, Ny, Nz = (t.to(dev) for t in (fem.Nvalues, fem.dN_x_values, fem.dN_y_values, fem.dN_z_values))       # (1, nbf, ngp, 1, 1, 1)
    jxw = (fem.gpw.to(dev) * wscale).reshape(1, 1, -1, 1, 1, 1)

    def weak(a_x, a_y, a_z, a_0):
        t = Nx * a_x.unsqueeze(1) + Ny * a_y.unsqueeze(1) + Nz * a_z.unsqueeze(1) + N * a_0.unsqueeze(1)
        return torch.sum(t * jxw, 2)

    return weak
