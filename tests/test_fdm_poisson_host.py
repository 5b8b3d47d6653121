"""CPU checks of the fused 2-D finite-difference Poisson residual (dn_fdm_poisson_apply, csrc/fdm_poisson.hip): the C ABI and its ctypes
binding agree and the library validates its arguments before any launch; the reference fixtures (tests/golden/loss_fdm_poisson_*.npz,
written by tools/gen_golden_fdm_poisson.py from the reference scripts' own `loss` bodies) agree with a float64 restatement of the
operator kept here -- residual, sums and the gradient by the hand-derived pullback of the header, not by autograd -- and with the
composed torch twin on the CPU; the pullback agrees with central differences; the default kernels are the reference's sobel* parameters.

The restatement (`restate`) also evaluates the operator "in absolute values" -- the same expression with every product replaced by its
absolute value -- which is the scale A of the rounding bounds  |fp32 result - float64| <= k 2^-24 A  used here and in
tests/test_gpu_fdm_poisson.py.  The chain lengths k (K_RES, K_GRAD) are derived in that module's docstring, for the kernel's order of
operations; the reference's own fp32 arithmetic (conv2d dot products of nine terms, the same elementwise passes, autograd's transposed
convolutions) has chains no longer than the kernel's, so the same k bound the fixtures."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from test_stokes_host import header_struct

FIXTURES = {"mms": "loss_fdm_poisson_mms_n9.npz", "klsum": "loss_fdm_poisson_klsum_n12.npz", "klsum_nbc": "loss_fdm_poisson_klsum_nbc_n9.npz"}
U24 = 2.0 ** -24
K_RES, K_GRAD = 22, 64                       # rounding chains of the residual and of the gradient (tests/test_gpu_fdm_poisson.py)


# ---------------------------------------------------------------------------------------------
# the float64 restatement
# ---------------------------------------------------------------------------------------------
def substitute(u, masks, vals):
    """u~ (float64) and the Dirichlet nodes: the conditions applied in order, fp32 masks compared with 0.5, others with zero."""
    ut, fixed = np.asarray(u, np.float64).copy(), np.zeros(u.shape, bool)
    for m, v in zip(masks, vals):
        if m is None:
            continue
        m = np.asarray(m)
        cond = np.broadcast_to(m > 0.5 if m.dtype.kind == "f" else m != 0, u.shape)
        ut = np.where(cond, np.broadcast_to(np.asarray(v, np.float64), u.shape), ut)
        fixed = fixed | cond
    return ut, fixed


def corr(v, k, absolute=False):
    """valid 3x3 correlation over the last two axes (nn.functional.conv2d); absolute: sum of |k v|"""
    ny, nx = v.shape[-2:]
    out = 0.0
    for a in range(3):
        for b in range(3):
            t = k[a, b] * v[..., a:ny - 2 + a, b:nx - 2 + b]
            out = out + (np.abs(t) if absolute else t)
    return out


def corr_t(w, k, shape, absolute=False):
    """the adjoint of corr: node j gathers k[j - i] w_i from the interior nodes i within one step of it"""
    ny, nx = shape[-2:]
    g = np.zeros(shape)
    for a in range(3):
        for b in range(3):
            t = k[a, b] * w
            g[..., a:ny - 2 + a, b:nx - 2 + b] += np.abs(t) if absolute else t
    return g


def restate(u, nu=1.0, f=0.0, fs=1.0, ks=None, masks=(), vals=(), out_scale=1.0, nbc_scale=0.0, in_scale=None, absolute=False):
    """(res (B,1,ny-2,nx-2), sums (B,3), grad (B,1,ny,nx)) of dn_fdm_poisson_args in float64, grad by the pullback derived by hand:
    d(sum r^2)/du~_j = 2 sum_i r_i (kx[j-i] (kx*nu)_i + ky[j-i] (ky*nu)_i + nu_i (kxx + kyy)[j-i]).  absolute: every product replaced
    by its absolute value (differences by sums of absolute values): the scale of the rounding bounds."""
    ab = absolute
    kx, ky, kxx, kyy = (np.asarray(k, np.float64).reshape(3, 3) for k in ks)
    ut, fixed = substitute(u, masks, vals)
    B = u.shape[0]
    nu = np.broadcast_to(np.asarray(nu, np.float64), u.shape)
    f = np.broadcast_to(np.asarray(f, np.float64), u.shape)
    pos = np.abs if ab else (lambda x: x)
    ux, uy, lap = corr(ut, kx, ab), corr(ut, ky, ab), corr(ut, kxx, ab) + corr(ut, kyy, ab)
    nux, nuy = corr(nu, kx, ab), corr(nu, ky, ab)
    nui, fi = pos(nu[..., 1:-1, 1:-1]), f[..., 1:-1, 1:-1]
    r = pos(fs * fi) + ux * nux + uy * nuy + nui * lap
    if ab:
        d0, d1 = np.abs(ut[:, :, 0]) + np.abs(ut[:, :, 1]), np.abs(ut[:, :, -1]) + np.abs(ut[:, :, -2])
    else:
        d0, d1 = ut[:, :, 0] - ut[:, :, 1], ut[:, :, -1] - ut[:, :, -2]
    sums = np.stack([(r ** 2).sum((1, 2, 3)), (d0 ** 2).sum((1, 2)), (d1 ** 2).sum((1, 2))], 1)
    gS = 2.0 * (corr_t(r * nux, kx, u.shape, ab) + corr_t(r * nuy, ky, u.shape, ab) + corr_t(r * nui, kxx, u.shape, ab)
                + corr_t(r * nui, kyy, u.shape, ab))
    gN = np.zeros(u.shape)
    sgn = 1.0 if ab else -1.0
    gN[:, :, 0] += 2.0 * d0
    gN[:, :, 1] += sgn * 2.0 * d0
    gN[:, :, -1] += 2.0 * d1
    gN[:, :, -2] += sgn * 2.0 * d1
    s = 1.0 if in_scale is None else np.asarray(in_scale, np.float64).reshape(B, 1, 1, 1)
    grad = pos(out_scale) * (pos(s) * gS + pos(nbc_scale) * gN)
    grad = np.where(fixed, 0.0, grad)
    return r, sums, grad


def script_loss(case, u, nu, f, ks, masks, vals):
    """What the three scripts minimise (the mean of the tensor their `loss` returns), its gradient, and the rounding bounds of both for
    fp32 arithmetic with the chains K_RES / K_GRAD: (loss, loss_bound, grad, grad_bound) in float64."""
    B, _, ny, nx = u.shape
    nin = (ny - 2) * (nx - 2)
    fs = 1.0 if case == "mms" else 0.0
    c = 0.1 if case == "klsum_nbc" else 0.0
    r, s, _ = restate(u, nu, f, fs, ks, masks, vals)
    ra, sa, _ = restate(u, nu, f, fs, ks, masks, vals, absolute=True)
    if case == "mms":                         # mean over the samples of ||r_b||_2
        nrm, nrma = np.sqrt(s[:, 0]), np.sqrt(sa[:, 0])
        loss = nrm.mean()
        # d||r|| <= ||dr|| <= K_RES u ||A_r||; the sum of squares n / 2 relative roundings after the square root, the root and the mean 2
        eps_nrm = (K_RES + nin / 2 + 2) * U24 * nrma
        loss_bound = eps_nrm.mean()
        kw = dict(out_scale=1.0 / B, in_scale=0.5 / nrm)
        _, _, grad = restate(u, nu, f, fs, ks, masks, vals, **kw)
        _, _, ga = restate(u, nu, f, fs, ks, masks, vals, absolute=True, **kw)
        # the gradient of sum r^2 over 2 ||r||: its own chain plus the relative error of the norm
        grad_bound = U24 * ga * (K_GRAD + (eps_nrm / U24 / nrm).reshape(B, 1, 1, 1))
    else:                                     # mean(r^2) (+ c mean over samples and x of the two Neumann row terms)
        loss = s[:, 0].sum() / (B * nin) + c * (s[:, 1] + s[:, 2]).sum() / (B * nx)
        loss_bound = U24 * ((2 * K_RES + 1 + B * nin) * sa[:, 0].sum() / (B * nin) + c * (4 + B * nx) * (sa[:, 1] + sa[:, 2]).sum() / (B * nx))
        kw = dict(out_scale=1.0 / (B * nin), nbc_scale=c * nin / nx)
        _, _, grad = restate(u, nu, f, fs, ks, masks, vals, **kw)
        _, _, ga = restate(u, nu, f, fs, ks, masks, vals, absolute=True, **kw)
        grad_bound = K_GRAD * U24 * ga
    return loss, loss_bound, grad, grad_bound


def load_fixture(case):
    z = np.load(os.path.join(GOLDEN, FIXTURES[case]))
    inp = z["inputs"]
    nu, bc1, bc2 = inp[:, 0:1], inp[:, 1:2], inp[:, 2:3]
    masks, vals = ((None, bc2), (0.0, 0.0)) if case == "mms" else ((bc1, bc2), (1.0, 0.0))      # 12_fdm_mms.py applies bc2 only
    ks = tuple(z[k].reshape(3, 3) for k in ("sobelx", "sobely", "sobelxx", "sobelyy"))
    return z, z["u"], nu, z["forcing"], ks, masks, vals


def method_args(case, nu, f, masks, vals, conv=lambda a: a):
    """The keyword arguments of DiffNetFDM.poisson_residual_loss (and its composed twin) that reproduce the script `case`."""
    return dict(nu=conv(nu), f=conv(f) if case == "mms" else None, bc=tuple(None if m is None else conv(m) for m in masks), bc_values=vals,
                norm="l2" if case == "mms" else "mean_sq", fs=1.0, neumann=0.1 if case == "klsum_nbc" else 0.0)


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_fdm_poisson_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    header = open(os.path.join(ROOT, "include", "diffnet_hip.h")).read()
    for s, proto in (("dn_fdm_poisson_workspace_bytes", "int64_t dn_fdm_poisson_workspace_bytes(int32_t B, int32_t ny, int32_t nx);"),
                     ("dn_fdm_poisson_apply", "int dn_fdm_poisson_apply(const dn_fdm_poisson_args *args, void *stream);")):
        assert hasattr(h, s) and s in _lib.SYMBOLS and proto in header, s
    assert _lib.SYMBOLS["dn_fdm_poisson_workspace_bytes"] == (C.c_int64, [C.c_int32] * 3)
    assert _lib.SYMBOLS["dn_fdm_poisson_apply"] == (C.c_int, [C.POINTER(_lib.DnFdmPoissonArgs), C.c_void_p])
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    assert "fdm_poisson.hip" in build.SOURCES
    got = [(n, getattr(t, "_length_", 1)) for n, t in _lib.DnFdmPoissonArgs._fields_]
    assert got == header_struct("dn_fdm_poisson_args")
    # the C layout (x86-64): 3 words + padding, 3 pointers, 2 words, 3 floats + padding, 2 x 40 bytes of conditions, 38 floats, 4 pointers,
    # a pointer and an int64
    assert _lib.DnFdmPoissonArgs.u.offset == 16 and _lib.DnFdmPoissonArgs.bc.offset == 64 and _lib.DnFdmPoissonArgs.kx.offset == 144
    assert _lib.DnFdmPoissonArgs.in_scale.offset == 296 and C.sizeof(_lib.DnFdmPoissonArgs) == 344


def fdm_args(B=2, ny=9, nx=11):
    from diffnet_amd import _lib
    a = _lib.DnFdmPoissonArgs()
    a.B, a.ny, a.nx = B, ny, nx
    return a


def test_fdm_poisson_workspace_bytes_and_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    ws = h.dn_fdm_poisson_workspace_bytes
    assert ws(2, 9, 11) == 64 * 65 + 24 * 1 * 9 * 2                 # the header + three doubles per (chunk, row, sample)
    assert ws(3, 7, 61) == 64 * 65 + 24 * 2 * 7 * 3                 # 60 owner columns per wave
    for bad in ((0, 9, 9), (65536, 9, 9), (1, 2, 9), (1, 9, 2), (1, -1, 9)):
        assert ws(*bad) == -1, bad
    apply = h.dn_fdm_poisson_apply
    assert apply(None, None) == -1
    a = fdm_args()
    a.grad = 64                                     # a NULL u
    assert apply(C.byref(a), None) == -1
    a.grad, a.u = None, 16                          # a field but no output at all: rejected before anything touches the pointers
    assert apply(C.byref(a), None) == -1
    for ny, nx in ((2, 9), (9, 2), (0, 9)):         # fewer than three nodes along an axis: no interior
        b = fdm_args(2, ny, nx)
        b.u, b.grad = 16, 64
        assert apply(C.byref(b), None) == -1, (ny, nx)
    b = fdm_args(0)
    b.u, b.grad = 16, 64
    assert apply(C.byref(b), None) == -1
    a.sums = 128                                    # sums without a workspace
    assert apply(C.byref(a), None) == -3
    a.workspace, a.workspace_bytes = 256, 64        # ... or with one that is too small
    assert apply(C.byref(a), None) == -3
    a.workspace_bytes = ws(2, 9, 11) - 1
    assert apply(C.byref(a), None) == -3
    a.sums, a.workspace, a.workspace_bytes = None, None, 0
    a.res = 64
    for k in (0, 1):
        for kind in (_lib.MASK_BITS, _lib.MASK_BOX):
            a.bc[k].mask_kind = kind
            assert apply(C.byref(a), None) == -2, (k, kind)
            a.bc[k].mask, a.bc[k].box_faces = 512, 15
            assert apply(C.byref(a), None) == -2, (k, kind)
            a.bc[k].mask, a.bc[k].box_faces = None, 0
        a.bc[k].mask_kind = 7
        assert apply(C.byref(a), None) == -1
        a.bc[k].mask_kind = 0
        a.bc[k].field = 120                         # a value field without its mask
        assert apply(C.byref(a), None) == -1
        a.bc[k].field = None
        for flag in ("mask_batched", "field_batched"):
            setattr(a.bc[k], flag, 2)
            assert apply(C.byref(a), None) == -1, flag
            setattr(a.bc[k], flag, 0)
    for flag in ("nu_batched", "f_batched"):
        setattr(a, flag, 2)
        assert apply(C.byref(a), None) == -1, flag
        setattr(a, flag, -1)
        assert apply(C.byref(a), None) == -1, flag
        setattr(a, flag, 0)


def test_fdm_poisson_op_refuses_cpu_tensors_and_bad_arguments():
    from diffnet_amd import ops
    from diffnet_amd._lib import DiffNetHipError
    u = torch.zeros(1, 1, 5, 5)
    with pytest.raises(DiffNetHipError):
        ops.fdm_poisson_apply(u)
    with pytest.raises(ValueError):
        ops.fdm_poisson_apply(u, want_res=False, want_grad=False, want_sums=False)
    with pytest.raises(ValueError):
        ops.fdm_poisson_apply(u, kernels=(np.zeros((3, 3)),) * 3)
    with pytest.raises(ValueError):
        ops.fdm_poisson_apply(u, bc_values=(0.0,))


# ---------------------------------------------------------------------------------------------
# the fixtures, the restatement, the composed twin
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(FIXTURES))
def test_restatement_reproduces_the_reference_fixture(case):
    z, u, nu, f, ks, masks, vals = load_fixture(case)
    loss, lb, grad, gb = script_loss(case, u, nu, f, ks, masks, vals)
    assert abs(float(z["loss_mean"]) - loss) <= lb, (float(z["loss_mean"]), loss, lb)
    err = np.abs(z["grad"].astype(np.float64) - grad)
    assert (err <= gb).all(), float((err / np.maximum(gb, 1e-300)).max())
    # the tensor the body returns: ||r_b|| (mms), r^2 (klsum), r^2 + 0.1 x the Neumann mean (klsum_nbc; B = 1)
    fs, c, nx = 1.0 if case == "mms" else 0.0, 0.1 if case == "klsum_nbc" else 0.0, u.shape[3]
    r, s, _ = restate(u, nu, f, fs, ks, masks, vals)
    ra, sa, _ = restate(u, nu, f, fs, ks, masks, vals, absolute=True)
    if case == "mms":
        want, bound = np.sqrt(s[:, 0]), (K_RES + r[0].size / 2 + 2) * U24 * np.sqrt(sa[:, 0])
    else:
        want = r[:, 0] ** 2 + c * (s[0, 1] + s[0, 2]) / nx
        bound = U24 * ((2 * K_RES + 2) * ra[:, 0] ** 2 + c * (4 + nx) * (sa[0, 1] + sa[0, 2]) / nx)
    assert z["loss"].shape == want.shape
    assert (np.abs(z["loss"] - want) <= bound).all()


@pytest.mark.parametrize("case", sorted(FIXTURES))
def test_composed_twin_reproduces_the_reference_fixture_on_the_cpu(case):
    from diffnet_amd.fdm import DiffNetFDM
    z, u, nu, f, ks, masks, vals = load_fixture(case)
    loss64, lb, grad64, gb = script_loss(case, u, nu, f, ks, masks, vals)
    m = DiffNetFDM(None, domain_size=int(z["n"]))
    ut = torch.tensor(u, requires_grad=True)
    loss = m.composed_poisson_residual_loss(ut, **method_args(case, nu, f, masks, vals, torch.tensor))
    g, = torch.autograd.grad(loss, ut)
    # both the twin and the fixture lie within the bound of float64
    loss = loss.detach()
    assert abs(float(loss) - loss64) <= lb and abs(float(loss) - float(z["loss_mean"])) <= 2 * lb
    assert (np.abs(g.numpy().astype(np.float64) - grad64) <= gb).all()
    assert (np.abs(g.numpy().astype(np.float64) - z["grad"]) <= 2 * gb).all()


def test_default_kernels_are_the_reference_parameters_bitwise():
    from diffnet_amd import ops
    from diffnet_amd.fdm import DiffNetFDM
    for case in sorted(FIXTURES):
        z = np.load(os.path.join(GOLDEN, FIXTURES[case]))
        n = int(z["n"])
        ks = ops.fdm_default_kernels(n)
        m = DiffNetFDM(None, domain_size=n)
        for k, name, par in zip(ks, ("sobelx", "sobely", "sobelxx", "sobelyy"), m._loss_kernels()):
            ref = z[name]
            assert ref.dtype == np.float32 and ref.shape == (1, 1, 3, 3)
            assert np.array_equal(np.asarray(k, np.float32).view(np.uint32), ref.reshape(-1).view(np.uint32)), (case, name)
            assert tuple(par) == tuple(k)
            assert np.array_equal(getattr(m, name).numpy().view(np.uint32), ref.view(np.uint32))


# ---------------------------------------------------------------------------------------------
# the pullback
# ---------------------------------------------------------------------------------------------
def test_hand_derived_pullback_matches_central_differences():
    rng = np.random.default_rng(7)
    B, ny, nx = 2, 6, 7
    u, nu, f = rng.standard_normal((B, 1, ny, nx)), 1.0 + rng.random((B, 1, ny, nx)), rng.standard_normal((1, 1, ny, nx))
    ks = tuple(rng.standard_normal((3, 3)) for _ in range(4))
    m0 = (rng.random((1, 1, ny, nx)) < 0.2).astype(np.float32)
    m1 = (rng.random((B, 1, ny, nx)) < 0.15).astype(np.uint8)
    m0[0, 0, 0, 2] = m1[1, 0, 1, 3] = m1[0, 0, ny - 1, 4] = 1             # conditions on the Neumann rows too
    vals = (0.7, rng.standard_normal((B, 1, ny, nx)))
    s_b = np.array([0.8, 1.7])
    kw = dict(nu=nu, f=f, fs=0.6, ks=ks, masks=(m0, m1), vals=vals, out_scale=0.37, nbc_scale=2.5, in_scale=s_b)

    def loss(v):
        _, s, _ = restate(v, **kw)
        return 0.37 * ((s_b * s[:, 0]).sum() + 2.5 * (s[:, 1] + s[:, 2]).sum())

    _, _, grad = restate(u, **kw)
    _, fixed = substitute(u, (m0, m1), vals)
    assert fixed.any() and not fixed.all() and (grad[fixed] == 0.0).all()
    h = 1e-3                                  # the loss is quadratic in u: central differences are exact up to rounding
    num = np.zeros_like(u)
    for idx in np.ndindex(*u.shape):
        up, um = u.copy(), u.copy()
        up[idx] += h
        um[idx] -= h
        num[idx] = (loss(up) - loss(um)) / (2 * h)
    np.testing.assert_allclose(grad, num, rtol=0, atol=1e-9 * max(1.0, np.abs(grad).max()))
