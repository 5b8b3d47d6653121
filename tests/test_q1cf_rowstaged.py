"""The row-staged closed-form 2-D Q1 element (diffnet_amd/csrc/poisson_elem.h: q1cf_stage / q1cf_elem; poisson2d_q1_cf.hip) without a GPU.

1. Its formulas restated in NumPy, in float64 and float32, against the oracle's energy + autograd gradient and its assembled residual:
   rules of 2, 3 and 4 points (the truncated 3- and 4-point literals included), square meshes and rectangular ones with hx != hy, with and
   without nu and f, energy (alpha = 2 c, beta = 1; and c = 0, where alpha = 0) and residual (alpha = beta = 1) scalings.
   float64: the restatement is the same polynomial as the Gauss sum, so it is held to 1e-12 -- against the oracle's FORMULATION with its
   tables as exact float64 tensor products (the stock tables are products rounded to float32 on store, 6e-8 off a tensor product; the
   closed form takes the 1-D rule, as the kernel does), and beside it against the stock oracle at 1e-6.  float32: against the stock oracle at the suite's tolerances (test_gpu_parity.py:
   scalars rtol 1e-5, gradients rtol 1e-4 + 1e-4 max|ref|, residual fields rtol 1e-5 + 1e-6 max|ref|).
2. A stand-alone host program (tests/host/q1cf_rowstaged_host.cpp) that marches a mesh with the kernel's own inline functions, built with
   the host side of hipcc, on the same inputs and tolerances.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from oracle.fem_oracle import Oracle, basis_1d, gauss_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------
# constants as dn_poisson_apply folds them (poisson_fused.hip): in double, rounded once to the working type
# ---------------------------------------------------------------------------------------------
def constants(ngp, hx, hy, alpha, beta, ws, dtype):
    x, w = gauss_rule(ngp)
    if dtype == np.float32:          # the library receives the 1-D rule as float32 (dn_mesh.gpw / basis)
        w = w.astype(np.float32).astype(np.float64)
        b = (0.5 * (1.0 + x)).astype(np.float32).astype(np.float64)
    else:
        b = 0.5 * (1.0 + x)
    mm = [float(np.sum(w * b ** r)) for r in range(4)]
    rr = np.array([mm[0] - 3 * mm[1] + 3 * mm[2] - mm[3], mm[1] - 2 * mm[2] + mm[3], mm[2] - mm[3], mm[3]])
    cc = np.array([mm[0] - 2 * mm[1] + mm[2], mm[1] - mm[2], mm[2]])
    k = dict(xm=rr / hx ** 2, ym=rr / hy ** 2 * ws, px=np.array([(mm[0] - mm[1]) * ws, mm[1] * ws]),
             sy=np.array([mm[0] - mm[1], mm[1]]), pn0=np.array(mm[0] * ws), s0=np.array(mm[0]), cx=cc * ws, cy=cc,
             ab=np.array([alpha, -beta]))
    return {n: v.astype(dtype) for n, v in k.items()}


def rowstaged(u, nu, f, k):
    """The kernel's arithmetic on whole arrays (B, ny, nx) of one dtype: returns e1 = sum W nu |grad u|^2, e2 = sum W f u, nodal contributions."""
    dt = u.dtype
    g = np.zeros_like(u)
    du = u[:, :, 1:] - u[:, :, :-1]                                                  # staged per node row
    pn = k["px"][0] * nu[:, :, :-1] + k["px"][1] * nu[:, :, 1:] if nu is not None else np.full_like(du, k["pn0"])
    V = u[:, 1:] - u[:, :-1]                                                         # per node and layer
    S = k["sy"][0] * nu[:, :-1] + k["sy"][1] * nu[:, 1:] if nu is not None else np.full_like(V, k["s0"])
    a, b, p, q = du[:, :-1], du[:, 1:], pn[:, :-1], pn[:, 1:]
    V0, V1, S0, S1 = V[:, :, :-1], V[:, :, 1:], S[:, :, :-1], S[:, :, 1:]
    xm, ym = k["xm"], k["ym"]
    X0, X1, X2 = p * xm[0] + q * xm[1], p * xm[1] + q * xm[2], p * xm[2] + q * xm[3]
    ta, tb = a * X0 + b * X1, a * X1 + b * X2
    Y0, Y1, Y2 = S0 * ym[0] + S1 * ym[1], S0 * ym[1] + S1 * ym[2], S0 * ym[2] + S1 * ym[3]
    t0, t1 = V0 * Y0 + V1 * Y1, V0 * Y1 + V1 * Y2
    e1 = np.sum((a * ta + b * tb + V0 * t0 + V1 * t1).astype(np.float64))
    al, nb = k["ab"]
    g[:, :-1, :-1] -= al * (ta + t0)
    g[:, :-1, 1:] += al * (ta - t1)
    g[:, 1:, :-1] += al * (t0 - tb)
    g[:, 1:, 1:] += al * (tb + t1)
    e2 = 0.0
    if f is not None:
        gx = np.zeros_like(u)                                                        # x-stage of the forcing, per node row
        gx[:, :, :-1] += k["cx"][0] * f[:, :, :-1] + k["cx"][1] * f[:, :, 1:]
        gx[:, :, 1:] += k["cx"][1] * f[:, :, :-1] + k["cx"][2] * f[:, :, 1:]
        tlo = k["cy"][0] * gx[:, :-1] + k["cy"][1] * gx[:, 1:]
        tup = k["cy"][1] * gx[:, :-1] + k["cy"][2] * gx[:, 1:]
        g[:, :-1] += nb * tlo
        g[:, 1:] += nb * tup
        e2 = np.sum((u[:, :-1] * tlo + u[:, 1:] * tup).astype(np.float64))
    assert g.dtype == dt
    return e1, e2, g


# ---------------------------------------------------------------------------------------------
# the oracle: stock (float32-rounded tables, evaluated in float64) and with exact float64 tensor-product tables
# ---------------------------------------------------------------------------------------------
def oracle64(kw, exact):
    o = Oracle(**kw)
    o.t = {n: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for n, v in o.t.items()}
    if exact:
        s = o.spec
        ng = s.ngp_1d
        Bs = [basis_1d(1, float(x)) for x in s.gpx_1d]
        sx = [2.0 / h for h in s.hs]
        K = {n: np.zeros((ng * ng, 2, 2)) for n in ("N_gp", "dN_x_gp", "dN_y_gp")}
        gpw = np.zeros(ng * ng)
        for jg in range(ng):
            for ig in range(ng):
                g = ng * jg + ig
                gpw[g] = s.gpw_1d[ig] * s.gpw_1d[jg]
                (bi, di, _), (bj, dj, _) = Bs[ig], Bs[jg]
                for jb in range(2):
                    for ib in range(2):
                        K["N_gp"][g, jb, ib] = bi[ib] * bj[jb]
                        K["dN_x_gp"][g, jb, ib] = di[ib] * bj[jb] * sx[0]
                        K["dN_y_gp"][g, jb, ib] = bi[ib] * dj[jb] * sx[1]
        for n, vn in (("N_gp", "Nvalues"), ("dN_x_gp", "dN_x_values"), ("dN_y_gp", "dN_y_values")):
            o.t[n] = torch.from_numpy(K[n].reshape(ng * ng, 1, 1, 2, 2))
            o.t[vn] = torch.from_numpy(np.ascontiguousarray(K[n].reshape(ng * ng, 4).T).reshape(1, 4, ng * ng, 1, 1))
        o.t["gpw"] = torch.from_numpy(gpw)
    o.gpw = o.t["gpw"]
    return o


def make_kw(ngp, sizes):
    nx, ny = sizes
    if nx == ny:
        return dict(domain_size=nx, ngp_1d=ngp)
    return dict(domain_size=nx, ngp_1d=ngp, domain_sizes=(nx, ny), domain_lengths=(0.02 * (nx - 1), 0.035 * (ny - 1)), domain_length=0.02 * (nx - 1))


def inputs(B, sizes, seed):
    nx, ny = sizes
    g = torch.Generator().manual_seed(seed)
    shape = (B, 1, ny, nx)
    u, nu, f = torch.rand(shape, generator=g, dtype=torch.float64), 0.5 + torch.rand(shape, generator=g, dtype=torch.float64), torch.rand(shape, generator=g, dtype=torch.float64)
    u, nu, f = (t.float().double() for t in (u, nu, f))            # representable in float32: both precisions see the same fields
    box = torch.zeros((1, 1, ny, nx), dtype=torch.float64)
    box[..., 0] = 1; box[..., -1] = 1; box[..., 0, :] = 1; box[..., -1, :] = 1
    obj = (torch.rand((1, 1, ny, nx), generator=g) < 0.06).double() * (1 - box)
    return u, nu, f, [(obj, 1.0), (box, 0.0)]


_REFS = {}


def reference(ngp, sizes, has_nu, has_f, exact):
    """Oracle energy + autograd gradient and assembled residual, computed once per case and shared (never modified)."""
    key = (ngp, sizes, has_nu, has_f, exact)
    if key not in _REFS:
        kw = make_kw(ngp, sizes)
        o = oracle64(kw, exact)
        u, nu, f, dl = inputs(2, sizes, 11 * ngp + sizes[0])
        a = dict(nu=nu if has_nu else None, f=f if has_f else None, dirichlet=dl)
        ur = u.clone().requires_grad_(True)
        e = o.energy(ur, c=0.5, jac=0.7, **a)
        (ge,) = torch.autograd.grad(e, ur)
        R = o.residual(u, jac=0.7, zero_masks=[m for m, _ in dl], **a)
        _REFS[key] = (o.spec, float(e.detach()), ge.numpy()[:, 0], R.numpy()[:, 0])
    return _REFS[key]


def applied(u, dl):
    keep = torch.ones_like(u[:1])
    for m, v in dl:
        u = torch.where(m > 0.5, v + u * 0.0, u)
        keep = keep * (1 - m)
    return u, keep


RULES = [2, 3, 4]
MESHES = [(12, 12), (13, 9)]
FIELDS = [(True, True), (True, False), (False, True), (False, False)]


def _evaluate(run, ngp, sizes, has_nu, has_f, dtype, exact):
    """Energy loss, its gradient and the residual from `run(u, nu, f, constants) -> e1, e2, g`, beside the oracle's."""
    spec, e_ref, ge_ref, R_ref = reference(ngp, sizes, has_nu, has_f, exact)
    u, nu, f, dl = inputs(2, sizes, 11 * ngp + sizes[0])
    ua, keep = applied(u, dl)
    arr = lambda t: np.ascontiguousarray(t.numpy()[:, 0].astype(dtype))
    un, nun, fn, kp = arr(ua), (arr(nu) if has_nu else None), (arr(f) if has_f else None), keep.numpy()[:, 0]
    hx, hy = spec.hs
    ws = 0.7
    nelem = 2 * spec.nel[0] * spec.nel[1]
    c = 0.5
    e1, e2, g = run(un, nun, fn, constants(ngp, hx, hy, 2.0 * c, 1.0, ws, dtype))
    energy = (c * e1 - e2) / nelem
    grad = g.astype(np.float64) * kp / nelem
    _, _, r = run(un, nun, fn, constants(ngp, hx, hy, 1.0, 1.0, ws, dtype))
    res = r.astype(np.float64) * kp
    # c = 0 (alpha = 0): the stiffness sum must still come out (the compliance-style losses read it), its cotangents vanish
    z1, z2, gz = run(un, nun, fn, constants(ngp, hx, hy, 0.0, 1.0, ws, dtype))
    np.testing.assert_allclose(z1, e1, rtol=1e-6)
    np.testing.assert_allclose(z2, e2, rtol=1e-6, atol=0 if has_f else 1e-30)
    _, _, g0 = run(un, None, fn, constants(ngp, hx, hy, 0.0, 1.0, ws, dtype)) if has_nu else (None, None, gz)
    np.testing.assert_array_equal(gz, g0)            # nothing of the stiffness term left in the nodal contributions
    return (energy, grad, res), (e_ref, ge_ref, R_ref)


def _check(got, ref, exact):
    (energy, grad, res), (e_ref, ge_ref, R_ref) = got, ref
    if exact:
        np.testing.assert_allclose(energy, e_ref, rtol=1e-12)
        np.testing.assert_allclose(grad, ge_ref, rtol=0, atol=1e-12 * np.abs(ge_ref).max())
        np.testing.assert_allclose(res, R_ref, rtol=0, atol=1e-12 * np.abs(R_ref).max())
    else:
        np.testing.assert_allclose(energy, e_ref, rtol=1e-5)
        np.testing.assert_allclose(grad, ge_ref, rtol=1e-4, atol=1e-4 * np.abs(ge_ref).max())
        np.testing.assert_allclose(res, R_ref, rtol=1e-5, atol=1e-6 * np.abs(R_ref).max())


@pytest.mark.parametrize("has_nu,has_f", FIELDS, ids=["nu_f", "nu", "f", "plain"])
@pytest.mark.parametrize("sizes", MESHES, ids=["12x12", "13x9"])
@pytest.mark.parametrize("ngp", RULES)
def test_float64_restatement_is_the_gauss_sum(ngp, sizes, has_nu, has_f):
    got, ref = _evaluate(rowstaged, ngp, sizes, has_nu, has_f, np.float64, True)
    _check(got, ref, True)
    # and against the STOCK oracle, which shows that the rebuilt tables are the oracle's own: its table entries are float64 products rounded
    # once to float32 (2^-24 = 6e-8 each); an energy term multiplies two derivative entries and a weight (3 x 6e-8), a residual entry two
    # entries and a weight, summed without cancellation beyond the field's own scale -> 1e-6 of the value / of the field's largest magnitude
    (energy, grad, res), (e_ref, ge_ref, R_ref) = _evaluate(rowstaged, ngp, sizes, has_nu, has_f, np.float64, False)
    np.testing.assert_allclose(energy, e_ref, rtol=1e-6)
    np.testing.assert_allclose(grad, ge_ref, rtol=0, atol=1e-6 * np.abs(ge_ref).max())
    np.testing.assert_allclose(res, R_ref, rtol=0, atol=1e-6 * np.abs(R_ref).max())


@pytest.mark.parametrize("has_nu,has_f", FIELDS, ids=["nu_f", "nu", "f", "plain"])
@pytest.mark.parametrize("sizes", MESHES, ids=["12x12", "13x9"])
@pytest.mark.parametrize("ngp", RULES)
def test_float32_restatement_within_suite_tolerances(ngp, sizes, has_nu, has_f):
    got, ref = _evaluate(rowstaged, ngp, sizes, has_nu, has_f, np.float32, False)
    _check(got, ref, False)


# ---------------------------------------------------------------------------------------------
# the kernel's own inline functions, in a host program
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    from diffnet_amd.build import _hipcc
    exe = str(tmp_path_factory.mktemp("q1cf_host") / "q1cf_rowstaged_host")
    cmd = [_hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=fast", "-I", os.path.join(ROOT, "diffnet_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "q1cf_rowstaged_host.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


def _host_run(exe, tmp):
    def run(u, nu, f, k):
        B, ny, nx = u.shape
        src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(src, "wb") as fh:
            fh.write(struct.pack("5i", B, ny, nx, int(nu is not None), int(f is not None)))
            for n in ("xm", "ym", "px", "sy", "pn0", "s0", "cx", "cy", "ab"):
                fh.write(np.asarray(k[n], dtype=np.float32).tobytes())
            for a in (u, nu, f):
                if a is not None:
                    fh.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
        subprocess.check_call([exe, src, dst])
        raw = open(dst, "rb").read()
        e1, e2 = struct.unpack("2d", raw[:16])
        g = np.frombuffer(raw[16:], dtype=np.float32).reshape(B, ny, nx).copy()
        return e1, e2, g
    return run


@pytest.mark.parametrize("has_nu,has_f", FIELDS, ids=["nu_f", "nu", "f", "plain"])
@pytest.mark.parametrize("sizes", MESHES, ids=["12x12", "13x9"])
@pytest.mark.parametrize("ngp", RULES)
def test_host_program_with_the_kernels_inline_functions(host_program, tmp_path, ngp, sizes, has_nu, has_f):
    got, ref = _evaluate(_host_run(host_program, str(tmp_path)), ngp, sizes, has_nu, has_f, np.float32, False)
    _check(got, ref, False)
    # and beside the float32 restatement: the same operations, other association and contraction only
    np_got, _ = _evaluate(rowstaged, ngp, sizes, has_nu, has_f, np.float32, False)
    np.testing.assert_allclose(got[0], np_got[0], rtol=2e-6)
    for a, b in zip(got[1:], np_got[1:]):
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-6 * np.abs(b).max())
