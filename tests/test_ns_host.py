"""CPU checks of the fused 2-D Navier-Stokes (VMS) residual (dn_ns_apply, csrc/navier_stokes.hip): the C ABI and its ctypes binding agree
and the library validates its arguments before any launch; the reference fixtures (tests/golden/loss_ns_*.npz, written by
tools/gen_golden_ns.py from the reference scripts' own residual bodies) agree with a float64 torch restatement of the operator kept here,
gradients included (autograd with tau detached); and the pointwise pullback the VJP launch implements, restated in numpy, equals the
restatement's autograd VJP."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_stokes_host import header_struct, q1_tables, stokes_mesh

FIXTURES = ["loss_ns_ldc_n17.npz", "loss_ns_ldc_n33_g3.npz", "loss_ns_fps_rect.npz"]


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_ns_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    for s in ("dn_ns_workspace_bytes", "dn_ns_apply"):
        assert hasattr(h, s) and s in _lib.SYMBOLS, s
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    got = [(n, getattr(t, "_length_", 1)) for n, t in _lib.DnNsArgs._fields_]
    assert got == header_struct("dn_ns_args")
    assert C.sizeof(_lib.DnNsArgs) == 272 and _lib.DnNsArgs.out.offset == 200          # the C layout (x86-64)


def test_ns_workspace_bytes_and_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    for ngp in (2, 3, 4):
        assert h.dn_ns_workspace_bytes(C.byref(stokes_mesh(ngp=ngp))) > 0
    assert h.dn_ns_workspace_bytes(C.byref(stokes_mesh(n=2049, B=8, ny=1025))) > 64 * 65
    for field, bad in (("nsd", 3), ("degree", 2), ("nx", 1), ("ny", 0), ("batch", 0), ("ngp", 5), ("ngp", 1)):
        m = stokes_mesh()
        setattr(m, field, bad)
        assert h.dn_ns_workspace_bytes(C.byref(m)) == -1, field
    m = stokes_mesh()
    assert h.dn_ns_apply(C.byref(m), None, None) == -1
    assert h.dn_ns_apply(None, None, None) == -1
    a = _lib.DnNsArgs()                             # no fields
    a.tau_h[0] = a.tau_h[1] = 0.1
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -1
    a.u, a.v, a.p = 16, 32, 48                      # fields but no output: rejected before anything touches the pointers
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -1
    a.out[0] = 64
    a.in_num = 80                                   # in_num without in_den
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -1
    a.in_den = 88                                   # both, but not in the VJP mode
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -1
    a.in_num = a.in_den = None
    a.vjp = 1                                       # a VJP without its cotangents
    a.cot[0], a.cot[1] = 96, 104
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -1
    a.vjp = 2
    a.cot[2] = 112
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -1
    a.vjp = 0
    a.mask_is_u8[1] = 2
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -1
    a.mask_is_u8[1] = 0
    a.bc_field[2] = 120                             # a value field without its mask
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -1
    a.bc_field[2] = None
    a.tau_h[1] = 0.0
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -1
    a.tau_h[1] = 0.1
    a.norms = 128                                   # a reduction without a workspace
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -3
    m.degree = 2
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -2
    m.degree, m.nsd = 1, 3
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -2
    m.nsd, m.ngp = 2, 5
    assert h.dn_ns_apply(C.byref(m), C.byref(a), None) == -2


def test_ns_ops_refuse_cpu_tensors_and_unsupported_meshes():
    from diffnet_amd import DiffNet2DFEM, ops
    from diffnet_amd._lib import DiffNetHipError
    from diffnet_amd.navier_stokes import ns_residuals
    m = DiffNet2DFEM(None, domain_size=9)
    u = torch.zeros((1, 1, 9, 9))
    with pytest.raises(DiffNetHipError):
        ops.ns_apply(m.geom, u, u, u)
    with pytest.raises(DiffNetHipError):
        ns_residuals(m, u, u, u, None)
    m2 = DiffNet2DFEM(None, domain_size=9, fem_basis_deg=2)
    with pytest.raises(DiffNetHipError):
        ops.ns_apply(m2.geom, u, u, u)


# ---------------------------------------------------------------------------------------------
# float64 restatement of the operator (include/diffnet_hip.h, dn_ns_args)
# ---------------------------------------------------------------------------------------------
def _tau_consts(visco, tau_h, cinv, dt=float):
    """(Gx, Gy, diffusion part, 1 / (gx^2 + gy^2)) as Python floats, the arithmetic in the type `dt`"""
    hx, hy, visco, cinv = dt(tau_h[0]), dt(tau_h[1]), dt(visco), dt(cinv)
    Gx, Gy = dt(4.0) / hx ** 2, dt(4.0) / hy ** 2
    out = Gx, Gy, cinv * visco ** 2 * (Gx ** 2 + Gy ** 2), dt(1.0) / (dt(4.0) / hx ** 2 + dt(4.0) / hy ** 2)
    assert all(isinstance(x, dt) for x in out)
    return tuple(float(x) for x in out)


def _np_type(dtype):
    """the numpy scalar type of a torch or numpy dtype"""
    return {torch.float64: np.float64, torch.float32: np.float32}.get(dtype) or np.dtype(dtype).type


def _q1_point_tables(N, dN, sx, sy, ig, jg, as_float=False):
    """N_a, Nx_a, Ny_a of the four local nodes (ly, lx) at Gauss point (ig, jg), in the type of the tables (as Python floats for torch)"""
    cv = float if as_float else (lambda x: x)
    Na = {(ly, lx): cv(N[ig, lx] * N[jg, ly]) for ly in (0, 1) for lx in (0, 1)}
    Nxa = {(ly, lx): cv(dN[ig, lx] * sx * N[jg, ly]) for ly in (0, 1) for lx in (0, 1)}
    Nya = {(ly, lx): cv(N[ig, lx] * dN[jg, ly] * sy) for ly in (0, 1) for lx in (0, 1)}
    return Na, Nxa, Nya


def _place(t, ly, lx):
    """an element array (nely, nelx) of local node (ly, lx) at its nodes (ny, nx)"""
    return torch.nn.functional.pad(t, (lx, 1 - lx, ly, 1 - ly))


def ns_torch(u, v, p, masks, vals, f1, f2, visco, J, hx, hy, tau_h, cinv, ngp, *, scale=False, dtype=torch.float64, tables=None):
    """u, v, p: (ny, nx) float64 tensors; masks[k]: bool arrays or None; vals[k]: float or (ny, nx); f1, f2: (G, nely, nelx), g = jg * ngp + ig.
    The scripts' weak forms term by term, tau from detached values.  Returns (R1, R2, R3), differentiable wrt u, v, p.
    dtype: the same statements in that type, with tables, constants and inputs cast once at entry; tables: the 1-D (N, dN, w) to use in
    place of q1_tables(ngp); scale: also returns (S1, S2, S3), S_k the sum of |w_g t| over the placed terms that make up the node's value
    (0 on the Dirichlet nodes of field k)."""
    dt = _np_type(dtype)
    N, dN, w = (np.asarray(t, dtype=dt) for t in (q1_tables(ngp) if tables is None else tables))
    u, v, p = (t.to(dtype) for t in (u, v, p))
    ny, nx = u.shape
    masks = [None if m is None else torch.as_tensor(m) for m in masks]
    vals = [torch.as_tensor(x, dtype=dtype) for x in vals]
    f1, f2 = torch.as_tensor(f1, dtype=dtype), torch.as_tensor(f2, dtype=dtype)
    fld = [t if m is None else torch.where(m, val.expand(ny, nx), t) for t, m, val in zip((u, v, p), masks, vals)]
    Gx, Gy, diff, gg_inv = _tau_consts(visco, tau_h, cinv, float if dt is np.float64 else dt)
    visco, J, sx, sy = float(dt(visco)), dt(J), dt(2) / dt(hx), dt(2) / dt(hy)
    R = [torch.zeros((ny, nx), dtype=dtype) for _ in range(3)]
    S = [torch.zeros((ny, nx), dtype=dtype) for _ in range(3)]
    for jg in range(ngp):
        for ig in range(ngp):
            g, wg = jg * ngp + ig, float(J * w[ig] * w[jg])
            Na, Nxa, Nya = _q1_point_tables(N, dN, sx, sy, ig, jg, as_float=True)

            def at(t, tab):
                return sum(tab[ly, lx] * t[ly:ny - 1 + ly, lx:nx - 1 + lx] for ly in (0, 1) for lx in (0, 1))

            uu, ux, uy = at(fld[0], Na), at(fld[0], Nxa), at(fld[0], Nya)
            vv, vx, vy = at(fld[1], Na), at(fld[1], Nxa), at(fld[1], Nya)
            pp, px, py = at(fld[2], Na), at(fld[2], Nxa), at(fld[2], Nya)
            a1, a2, d = uu * ux + vv * uy, uu * vx + vv * vy, ux + vy
            r1, r2 = a1 + px - f1[g], a2 + py - f2[g]
            temp = torch.sqrt(Gx * uu.detach() ** 2 + Gy * vv.detach() ** 2 + diff)
            tm, tc = 1.0 / temp, temp * gg_inv
            for (ly, lx), n_ in Na.items():
                nx_, ny_ = Nxa[ly, lx], Nya[ly, lx]
                t1 = (n_ * a1 + visco * (nx_ * ux + ny_ * uy) - nx_ * pp - n_ * f1[g] + tm * (uu * nx_ + vv * ny_) * r1
                      - tm * n_ * (r1 * ux + r2 * uy) - tm ** 2 * r1 * (r1 * nx_ + r2 * ny_) + tc * nx_ * d)
                t2 = (n_ * a2 + visco * (nx_ * vx + ny_ * vy) - ny_ * pp - n_ * f2[g] + tm * (uu * nx_ + vv * ny_) * r2
                      - tm * n_ * (r1 * vx + r2 * vy) - tm ** 2 * r2 * (r1 * nx_ + r2 * ny_) + tc * ny_ * d)
                t3 = n_ * d + tm * (nx_ * r1 + ny_ * r2)
                for k, t in enumerate((t1, t2, t3)):
                    R[k] = R[k] + _place(wg * t, ly, lx)
                    if scale:
                        S[k] = S[k] + _place((wg * t).detach().abs(), ly, lx)
    R = tuple(r if m is None else torch.where(m, val.expand(ny, nx), r) for r, m, val in zip(R, masks, vals))
    assert all(r.dtype == dtype for r in R), [r.dtype for r in R]
    if not scale:
        return R
    return R, tuple(s if m is None else torch.where(m, torch.zeros_like(s), s) for s, m in zip(S, masks))


def fixture_case(z):
    kw = eval(str(z["kwargs"]))
    sizes = kw.get("domain_sizes", (kw["domain_size"], kw["domain_size"]))[:2]
    lengths = kw.get("domain_lengths", (kw.get("domain_length", 1.0),) * 2)[:2]
    hx, hy = lengths[0] / (sizes[0] - 1), lengths[1] / (sizes[1] - 1)
    inp = z["inputs"].astype(np.float64)
    masks = [inp[0, 2 + k] >= 0.5 for k in range(3)]
    vals = [z[n].astype(np.float64) for n in ("u_bc", "v_bc", "p_bc")]
    return dict(masks=masks, vals=vals, f1=z["f1"].astype(np.float64), f2=z["f2"].astype(np.float64), visco=float(z["visco"]),
                J=float(z["wscale"]), hx=hx, hy=hy, tau_h=tuple(float(x) for x in z["tau_h"]), cinv=36.0, ngp=kw.get("ngp_1d", 2))


@pytest.mark.parametrize("name", FIXTURES)
def test_ns_fixtures_agree_with_float64_restatement(name):
    z = np.load(os.path.join(GOLDEN, name))
    c = fixture_case(z)
    fields = [torch.tensor(z[n][0, 0], dtype=torch.float64, requires_grad=True) for n in ("u", "v", "p")]
    R = ns_torch(*fields, **c)
    norms = [torch.linalg.norm(r) for r in R]
    for k in range(3):
        ref = z[f"R{k + 1}"][0, 0]
        np.testing.assert_allclose(R[k].detach().numpy(), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max(), err_msg=f"R{k + 1}")
        np.testing.assert_allclose(float(norms[k].detach()), z["norms"][k], rtol=1e-5)
        gs = torch.autograd.grad(norms[k], fields, retain_graph=True)
        ref = z[f"grad_norm{k + 1}"][:, 0, 0]
        for q in range(3):
            np.testing.assert_allclose(gs[q].numpy(), ref[q], rtol=1e-4, atol=1e-4 * np.abs(ref).max(),
                                       err_msg=f"grad of ||R{k + 1}|| wrt field {q}")


# ---------------------------------------------------------------------------------------------
# the pullback of the VJP launch (csrc/navier_stokes.hip: ns_vjp_flux), restated in numpy
# ---------------------------------------------------------------------------------------------
def ns_vjp_np(u, v, p, lam, masks, vals, f1, f2, visco, J, hx, hy, tau_h, cinv, ngp, *, scale=False, dtype=np.float64, tables=None):
    """d/d(u, v, p) of sum_k <lam_k, R_k> with tau held fixed: the cotangents (zeroed on the Dirichlet rows of their residual) evaluated
    like fields, the hand-derived pointwise coefficients, pulled back through N, Nx, Ny and zeroed on each field's Dirichlet nodes.
    scale, dtype, tables: as in ns_torch."""
    dt = np.dtype(dtype).type
    c = lambda x: np.asarray(x, dtype=dt)                                  # noqa: E731
    N, dN, w = (c(t) for t in (q1_tables(ngp) if tables is None else tables))
    u, v, p, f1, f2 = (c(x) for x in (u, v, p, f1, f2))
    lam, vals = [c(x) for x in lam], [c(x) for x in vals]
    ny, nx = u.shape
    fld = [t if m is None else np.where(m, val, t) for t, m, val in zip((u, v, p), masks, vals)]
    lam = [l_ if m is None else np.where(m, dt(0), l_) for l_, m in zip(lam, masks)]
    Gx, Gy, diff, gg_inv = (dt(x) for x in _tau_consts(visco, tau_h, cinv, float if dt is np.float64 else dt))
    visco, J, sx, sy = dt(visco), dt(J), dt(2) / dt(hx), dt(2) / dt(hy)
    out = [np.zeros((ny, nx), dtype=dt) for _ in range(3)]
    S = [np.zeros((ny, nx), dtype=dt) for _ in range(3)]
    for jg in range(ngp):
        for ig in range(ngp):
            g, wg = jg * ngp + ig, J * w[ig] * w[jg]
            Na, Nxa, Nya = _q1_point_tables(N, dN, sx, sy, ig, jg)

            def at(t, tab):
                return sum(tab[ly, lx] * t[ly:ny - 1 + ly, lx:nx - 1 + lx] for ly in (0, 1) for lx in (0, 1))

            uu, ux, uy = at(fld[0], Na), at(fld[0], Nxa), at(fld[0], Nya)
            vv, vx, vy = at(fld[1], Na), at(fld[1], Nxa), at(fld[1], Nya)
            px, py = at(fld[2], Nxa), at(fld[2], Nya)
            L = [at(x, Na) for x in lam]
            Lx = [at(x, Nxa) for x in lam]
            Ly = [at(x, Nya) for x in lam]
            a1, a2 = uu * ux + vv * uy, uu * vx + vv * vy
            r1, r2 = a1 + px - f1[g], a2 + py - f2[g]
            temp = np.sqrt(Gx * uu ** 2 + Gy * vv ** 2 + diff)
            tm, tc = 1.0 / temp, temp * gg_inv
            tm2 = tm * tm
            g1 = -tm * (L[0] * ux + L[1] * vx) + Lx[0] * (tm * uu - 2 * tm2 * r1) + Ly[0] * (tm * vv - tm2 * r2) - Lx[1] * tm2 * r2 + Lx[2] * tm
            g2 = -tm * (L[0] * uy + L[1] * vy) - Ly[0] * tm2 * r1 + Lx[1] * (tm * uu - tm2 * r1) + Ly[1] * (tm * vv - 2 * tm2 * r2) + Ly[2] * tm
            h1, h2, hd = L[0] + g1, L[1] + g2, L[2] + tc * (Lx[0] + Ly[1])
            coef = [(h1 * ux + h2 * vx + tm * (Lx[0] * r1 + Lx[1] * r2), h1 * uu - tm * r1 * L[0] + visco * Lx[0] + hd,
                     h1 * vv - tm * r2 * L[0] + visco * Ly[0]),
                    (h1 * uy + h2 * vy + tm * (Ly[0] * r1 + Ly[1] * r2), h2 * uu - tm * r1 * L[1] + visco * Lx[1],
                     h2 * vv - tm * r2 * L[1] + visco * Ly[1] + hd),
                    (-(Lx[0] + Ly[1]), g1, g2)]
            for (ly, lx), n_ in Na.items():
                for k, (A, B, Cc) in enumerate(coef):
                    t = wg * (n_ * A + Nxa[ly, lx] * B + Nya[ly, lx] * Cc)
                    out[k][ly:ny - 1 + ly, lx:nx - 1 + lx] += t
                    S[k][ly:ny - 1 + ly, lx:nx - 1 + lx] += np.abs(t)
    out = [o if m is None else np.where(m, dt(0), o) for o, m in zip(out, masks)]
    assert all(o.dtype == dt for o in out), [o.dtype for o in out]             # numpy promotes silently
    if not scale:
        return out
    return out, [s if m is None else np.where(m, dt(0), s) for s, m in zip(S, masks)]


@pytest.mark.parametrize("ngp,ny,nx", [(2, 6, 7), (3, 5, 6), (4, 4, 5)])
def test_ns_hand_pullback_equals_autograd_of_the_restatement(ngp, ny, nx):
    rs = np.random.default_rng(11 + ngp)
    fields = [2 * rs.random((ny, nx)) - 1 for _ in range(3)]
    lam = [2 * rs.random((ny, nx)) - 1 for _ in range(3)]
    masks = [rs.random((ny, nx)) < 0.3, rs.random((ny, nx)) < 0.3, None]
    G = ngp * ngp
    c = dict(masks=masks, vals=[0.3, 2 * rs.random((ny, nx)) - 1, 0.0], f1=rs.random((G, ny - 1, nx - 1)) - 0.5,
             f2=rs.random((G, ny - 1, nx - 1)) - 0.5, visco=0.05, J=0.02, hx=0.2, hy=0.25, tau_h=(0.2, 0.25), cinv=36.0, ngp=ngp)
    ft = [torch.tensor(f, requires_grad=True) for f in fields]
    R = ns_torch(*ft, **c)
    s = sum((r * torch.tensor(l_)).sum() for r, l_ in zip(R, lam))
    ref = torch.autograd.grad(s, ft)
    got = ns_vjp_np(*fields, lam, **c)
    for q in range(3):
        scale = float(ref[q].abs().max())
        assert scale > 1e-3
        np.testing.assert_allclose(got[q], ref[q].numpy(), rtol=0, atol=1e-12 * scale, err_msg=f"field {q}")
