"""Finite-difference operator class with the reference's surface (`DiffNet/DiffNetFDM.py`): `DiffNetFDM` with
`derivative_x / _y / _xx / _yy` on replicate-padded fields, the `sobel*` kernels, `h_corr / v_corr` correction matrices
and `pad / pad_d2` modules as attributes (state_dict keys preserved).  The arithmetic -- 3x3 stencil + boundary
fix-up, which the reference performs as conv2d followed by a dense N x N matmul -- is one HIP kernel per call
(`dn_fdm_stencil_fwd/bwd`).  Like the reference the class is hard-wired to nsd = 2, 'fdm' weights, 3-point stencils
(`DiffNetFDM.py:128-130`); its z-derivatives and `calc_laplacian` reference attributes that never exist there
 and raise here."""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable
from torch import nn

from . import _lib
from .base import PDE
from .ops import _p, _require, _stream


def get_deriv_kernels(nsd, ktype, num_pt, output_dim):
    """3-point kernels of DiffNetFDM.py:6-60 for nsd = 2 (first derivative: central difference x row-average)."""
    if nsd != 2 or num_pt != 3 or ktype not in ("fdm", "sobel"):
        raise NotImplementedError("only the configuration the reference class uses (nsd=2, 3-point, fdm/sobel) is built")
    stencil = np.array([-1.0, 0.0, 1.0], dtype=np.float32) * ((output_dim - 1) / 2.0)
    weights = np.array([1, 1, 1] if ktype == "fdm" else [1, 2, 1], dtype=np.float32)
    d2_stencil = ((output_dim - 1) ** 2) * np.array([1, -2, 1], dtype=np.float32)
    d2_weights = np.array([1, 1, 1], dtype=np.float32)
    ker_x = (np.kron(weights, stencil) / np.sum(weights)).reshape(3, 3)
    ker_xx = (np.kron(d2_weights, d2_stencil) / np.sum(d2_weights)).reshape(3, 3)
    return 1, ker_x, ker_x.T, np.zeros_like(ker_x), 1, ker_xx, ker_xx.T, np.zeros_like(ker_xx)


def get_sobel_correction_matrix(nsd, size, padding_xy, padding_xy_d2):
    """Boundary-correction matrices of DiffNetFDM.py:63-119 (padding 1): identity except the two corner 2x1 blocks."""
    w = size
    cm = np.eye(w, dtype=np.float32)
    cm[0, 0] = cm[w - 1, w - 1] = 4.0
    cm[1, 0] = cm[w - 2, w - 1] = -1.0
    cm2 = np.eye(w, dtype=np.float32)
    cm2[0, 0] = cm2[w - 1, w - 1] = 0.0
    cm2[1, 0] = cm2[w - 2, w - 1] = 1.0
    return cm, cm.T.copy(), cm2, cm2.T.copy()


class _Stencil(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, k9, axis, a, b):
        g = _require(g, "g", 4)
        if g.shape[1] != 1 or g.shape[2] < 3 or g.shape[3] < 3:
            raise ValueError(f"expected a replicate-padded single-channel field (B,1,N+2,N+2), got {tuple(g.shape)}")
        B, ny, nx = g.shape[0], g.shape[2] - 2, g.shape[3] - 2
        out = torch.empty((B, 1, ny, nx), dtype=torch.float32, device=g.device)
        karr = (C.c_float * 9)(*k9)
        rc = _lib.lib().dn_fdm_stencil_fwd(_p(g), _p(out), B, ny, nx, karr, axis, a, b, _stream(g))
        _lib.check(rc, "dn_fdm_stencil_fwd")
        ctx.meta = (k9, axis, a, b, B, ny, nx)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        k9, axis, a, b, B, ny, nx = ctx.meta
        go = _require(go, "grad_output", 4)
        gg = torch.empty((B, 1, ny + 2, nx + 2), dtype=torch.float32, device=go.device)
        karr = (C.c_float * 9)(*k9)
        rc = _lib.lib().dn_fdm_stencil_bwd(_p(go), _p(gg), B, ny, nx, karr, axis, a, b, _stream(go))
        _lib.check(rc, "dn_fdm_stencil_bwd")
        return gg, None, None, None, None


class _StencilFused(torch.autograd.Function):
    """pad + stencil + boundary fix-up in one launch each way (dn_fdm_fused_fwd/bwd): input and output on the same grid."""

    @staticmethod
    def forward(ctx, u, k9, axis, a, b):
        u = _require(u, "u", 4)
        if u.shape[1] != 1:
            raise ValueError(f"expected a single-channel field (B,1,N,N), got {tuple(u.shape)}")
        B, ny, nx = u.shape[0], u.shape[2], u.shape[3]
        out = torch.empty_like(u)
        rc = _lib.lib().dn_fdm_fused_fwd(_p(u), _p(out), B, ny, nx, (C.c_float * 9)(*k9), axis, a, b, _stream(u))
        _lib.check(rc, "dn_fdm_fused_fwd")
        ctx.meta = (k9, axis, a, b, B, ny, nx)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        k9, axis, a, b, B, ny, nx = ctx.meta
        go = _require(go, "grad_output", 4)
        gu = torch.empty_like(go)
        rc = _lib.lib().dn_fdm_fused_bwd(_p(go), _p(gu), B, ny, nx, (C.c_float * 9)(*k9), axis, a, b, _stream(go))
        _lib.check(rc, "dn_fdm_fused_bwd")
        return gu, None, None, None, None


def _bc_pair(bc):
    """The conditions of a loss call as a pair of masks: none, one mask, or up to two in a sequence (either may be None)."""
    if bc is None:
        return (None, None)
    if isinstance(bc, torch.Tensor):
        return (bc, None)
    bc = tuple(bc)
    if len(bc) > 2:
        raise ValueError(f"poisson_residual_loss: at most two conditions (got {len(bc)})")
    return bc + (None,) * (2 - len(bc))


class _PoissonResidualLoss(torch.autograd.Function):
    """DiffNetFDM.poisson_residual_loss: the fused loss; its gradient with respect to u is taken in the forward, by the same launch."""

    @staticmethod
    def forward(ctx, u, fdm, nu, f, bc, bc_values, norm, fs, neumann):
        loss, grad = fdm._poisson_loss_and_grad(u, nu, f, bc, bc_values, norm, fs, neumann, want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        grad, = ctx.saved_tensors
        return (grad * go,) + (None,) * 8


class DiffNetFDM(PDE):
    def __init__(self, network, dataset=None, **kwargs):
        super().__init__(network, dataset, **kwargs)
        self.nsd = 2
        self.ktype = 'fdm'
        self.stencil_len = 3
        p1, kx, ky, kz, p2, kxx, kyy, kzz = get_deriv_kernels(self.nsd, self.ktype, self.stencil_len, self.domain_size)
        cX, cY, cX2, cY2 = get_sobel_correction_matrix(self.nsd, self.domain_size, p1, p2)

        def par(a):
            return nn.Parameter(torch.tensor(np.ascontiguousarray(a, dtype=np.float32)).unsqueeze(0).unsqueeze(1), requires_grad=False)

        self.sobelx, self.sobely, self.sobelz = par(kx), par(ky), par(kz)
        self.sobelxx, self.sobelyy, self.sobelzz = par(kxx), par(kyy), par(kzz)
        self.h_corr, self.v_corr = par(cX), par(cY)
        self.h_corr_d2, self.v_corr_d2 = par(cX2), par(cY2)
        self.pad = nn.ReplicationPad2d(padding=p1)
        self.pad_d2 = nn.ReplicationPad2d(padding=p2)
        self._k = {n: tuple(float(v) for v in np.asarray(k, dtype=np.float32).reshape(-1)) for n, k in
                   (("x", kx), ("y", ky), ("xx", kxx), ("yy", kyy))}

    def derivative_x(self, g):
        return _Stencil.apply(g, self._k["x"], 0, 4.0, -1.0)

    def derivative_y(self, g):
        return _Stencil.apply(g, self._k["y"], 1, 4.0, -1.0)

    def derivative_xx(self, g):
        return _Stencil.apply(g, self._k["xx"], 0, 0.0, 1.0)

    def derivative_yy(self, g):
        return _Stencil.apply(g, self._k["yy"], 1, 0.0, 1.0)

    # fused level (new): the replicate padding the reference applies with `self.pad(u)` is folded into the kernel
    def dx(self, u):
        """== derivative_x(self.pad(u)) in one launch, no padded tensor."""
        return _StencilFused.apply(u, self._k["x"], 0, 4.0, -1.0)

    def dy(self, u):
        return _StencilFused.apply(u, self._k["y"], 1, 4.0, -1.0)

    def dxx(self, u):
        return _StencilFused.apply(u, self._k["xx"], 0, 0.0, 1.0)

    def dyy(self, u):
        return _StencilFused.apply(u, self._k["yy"], 1, 0.0, 1.0)

    # fused loss level (new): the whole residual loss of the reference's FDM scripts and its gradient (dn_fdm_poisson_apply)
    def _loss_kernels(self):
        return self._k["x"], self._k["y"], self._k["xx"], self._k["yy"]

    def _poisson_loss_and_grad(self, u, nu, f, bc, bc_values, norm, fs, neumann, want_grad=True):
        from . import ops
        if norm not in ("mean_sq", "l2"):
            raise ValueError(f"poisson_residual_loss: norm must be 'mean_sq' or 'l2' (the scripts keep their L1 term commented out), got {norm!r}")
        B, _, ny, nx = u.shape
        nin, neumann = (ny - 2) * (nx - 2), float(neumann)
        common = dict(nu=nu, f=f, bc=_bc_pair(bc), bc_values=bc_values, kernels=self._loss_kernels(), fs=fs)
        if norm == "mean_sq":                # mean(res^2) + neumann * mean_x(down^2 + up^2), averaged over the samples: one launch
            grad, s, _ = ops.fdm_poisson_apply(u, out_scale=1.0 / (B * nin), nbc_scale=neumann * nin / nx, want_grad=want_grad, **common)
            loss = s[:, 0].sum() / (B * nin)
        else:                                # mean over the samples of ||res_b||_2: the sums first, the gradient from them
            _, s, _ = ops.fdm_poisson_apply(u, want_grad=False, **common)
            nrm = torch.sqrt(s[:, 0])
            loss = nrm.mean()
            grad = None
            if want_grad:                    # d||r|| / du = d(sum r^2) / du / (2 ||r||); torch's convention at ||r|| == 0: zero
                half_inv = torch.where(nrm > 0, 0.5 / nrm, torch.zeros_like(nrm)).float()
                grad, _, _ = ops.fdm_poisson_apply(u, out_scale=1.0 / B, nbc_scale=neumann / nx, in_scale=half_inv, want_sums=False, **common)
        if neumann != 0.0:
            loss = loss + neumann * (s[:, 1] + s[:, 2]).sum() / (B * nx)
        return loss.float(), grad

    def poisson_residual_loss_and_grad(self, u, nu, f=None, bc=(), bc_values=(0.0, 0.0), norm="mean_sq", fs=1.0, neumann=0.0):
        """(loss, dloss/du) of the finite-difference Poisson residual loss, fused (ops.fdm_poisson_apply): with u~ the field after the
        conditions `bc` (none, one or two masks; u~ takes `bc_values[k]` under condition k, condition 2 wins) and the class's kernels,
            res = fs f + conv2d(u~, sobelx) conv2d(nu, sobelx) + conv2d(u~, sobely) conv2d(nu, sobely)
                  + nu[1:-1, 1:-1] (conv2d(u~, sobelxx) + conv2d(u~, sobelyy))
            norm "mean_sq":  mean(res^2)                      -- 12_klsum_fdm.py (its loss(...).mean()), one launch
            norm "l2":       mean over the samples of ||res_b||_2   -- 12_fdm_mms.py, two launches
            neumann c != 0:  + c * mean over samples and x of (u~[0] - u~[1])^2 + (u~[-1] - u~[-2])^2
        "mean_sq" with neumann = 0.1 is 12_klsum_fdm_nbc.py at B = 1: that script adds a (B, 1) Neumann term to a (B, N-2, N-2) residual,
        a broadcast that exists only for B = 1; for B > 1 this method averages the per-sample losses.  `nu`: tensor (B | 1,1,ny,nx),
        float or None (1); `f`: likewise (None: no forcing).  The loss is a float32 scalar on u's device."""
        return self._poisson_loss_and_grad(u, nu, f, bc, bc_values, norm, fs, neumann)

    def poisson_residual_loss(self, u, nu, f=None, bc=(), bc_values=(0.0, 0.0), norm="mean_sq", fs=1.0, neumann=0.0):
        """The loss of `poisson_residual_loss_and_grad`, differentiable with respect to u: `loss.backward()` works (the gradient is
        taken by the same launch as the loss, or by the second one of norm "l2", when u requires it)."""
        return _PoissonResidualLoss.apply(u, self, nu, f, bc, bc_values, norm, fs, neumann)

    def composed_poisson_residual_loss(self, u, nu, f=None, bc=(), bc_values=(0.0, 0.0), norm="mean_sq", fs=1.0, neumann=0.0):
        """The same loss from torch's own operators, as the reference's scripts compose it (torch.where, six conv2d calls, elementwise
        passes, autograd): any device, differentiable with respect to every tensor input.  The twin the fused loss is compared with."""
        conv = nn.functional.conv2d
        if not isinstance(nu, torch.Tensor):
            nu = torch.full_like(u[:1], 1.0 if nu is None else float(nu))
        if norm not in ("mean_sq", "l2"):
            raise ValueError(f"composed_poisson_residual_loss: norm must be 'mean_sq' or 'l2', got {norm!r}")
        for m, v in zip(_bc_pair(bc), bc_values):
            if m is not None:
                cond = m > 0.5 if m.dtype.is_floating_point else m.bool()
                u = torch.where(cond, v if isinstance(v, torch.Tensor) else u * 0.0 + float(v), u)
        lap = conv(u, self.sobelxx) + conv(u, self.sobelyy)
        res = conv(u, self.sobelx) * conv(nu, self.sobelx) + conv(u, self.sobely) * conv(nu, self.sobely) + nu[:, :, 1:-1, 1:-1] * lap
        if f is not None:
            res = fs * (f[:, :, 1:-1, 1:-1] if isinstance(f, torch.Tensor) else float(f)) + res
        res = res.reshape(u.shape[0], -1)
        loss = (res ** 2).mean() if norm == "mean_sq" else torch.norm(res, p=2, dim=1).mean()
        if float(neumann) != 0.0:
            nbc = (u[:, :, 0, :] - u[:, :, 1, :]) ** 2 + (u[:, :, -1, :] - u[:, :, -2, :]) ** 2
            loss = loss + float(neumann) * nbc.mean()
        return loss

    def derivative_z(self, g):
        raise NotImplementedError("the reference class is hard-wired to nsd = 2 (DiffNetFDM.py:128); z-derivatives are unreachable there")

    derivative_zz = derivative_z

    def calc_laplacian(self, g):
        raise AttributeError("'DiffNetFDM' object has no attribute 'laplacian' (same as the reference: DiffNetFDM.py:201-203)")
