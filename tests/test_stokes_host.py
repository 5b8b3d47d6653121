"""CPU checks of the fused 2-D Stokes (PSPG) residual (dn_stokes_apply, csrc/stokes.hip): the C ABI and its ctypes binding agree and the
library validates its arguments before any launch; the reference fixtures (tests/golden/loss_stokes_*.npz, written by
tools/gen_golden_stokes.py from the reference scripts' own residual bodies) agree with a float64 numpy restatement of the operator kept
here, and that restatement satisfies the adjoint identity the transpose launch relies on: J_R^T = S J_R S, S = diag(1, 1, -1)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

FIXTURES = ["loss_stokes_ldc_n17.npz", "loss_stokes_mms_n33_g3.npz", "loss_stokes_fps_rect.npz"]


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def header_struct(name):
    text = open(os.path.join(ROOT, "include", "diffnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in re.sub(r"^(const\s+)?\w+\s*", "", decl).split(","):
            m = re.match(r"\s*\**\s*(\w+)\s*(?:\[(\d+)\])?", part)
            fields.append((m.group(1), int(m.group(2) or 1)))
    return fields


def test_stokes_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    for s in ("dn_stokes_workspace_bytes", "dn_stokes_apply"):
        assert hasattr(h, s) and s in _lib.SYMBOLS, s
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    got = [(n, getattr(t, "_length_", 1)) for n, t in _lib.DnStokesArgs._fields_]
    assert got == header_struct("dn_stokes_args")
    assert C.sizeof(_lib.DnStokesArgs) == 240 and _lib.DnStokesArgs.out.offset == 168          # the C layout (x86-64)


def stokes_mesh(n=33, ngp=2, B=2, ny=None):
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    gx, gw = gauss_rule(ngp)
    ny = n if ny is None else ny
    return FemGeometry(2, (n, ny), (1 / (n - 1), 1 / (ny - 1)), 1, ngp, gx, gw).mesh_struct(B)


def test_stokes_workspace_bytes_and_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    for ngp in (2, 3, 4):
        m = stokes_mesh(ngp=ngp)
        assert h.dn_stokes_workspace_bytes(C.byref(m)) > 0
    m = stokes_mesh(n=2049, B=8, ny=1025)
    assert h.dn_stokes_workspace_bytes(C.byref(m)) > 64 * 65
    m = stokes_mesh()
    m.nsd, m.nz = 3, 5
    assert h.dn_stokes_workspace_bytes(C.byref(m)) == -1
    m = stokes_mesh()
    m.degree = 2
    assert h.dn_stokes_workspace_bytes(C.byref(m)) == -1
    for field, bad in (("nx", 1), ("ny", 0), ("batch", 0), ("ngp", 5), ("ngp", 1)):
        m = stokes_mesh()
        setattr(m, field, bad)
        assert h.dn_stokes_workspace_bytes(C.byref(m)) == -1, field
    m = stokes_mesh()
    assert h.dn_stokes_apply(C.byref(m), None, None) == -1
    assert h.dn_stokes_apply(None, None, None) == -1
    a = _lib.DnStokesArgs()                         # no fields
    assert h.dn_stokes_apply(C.byref(m), C.byref(a), None) == -1
    a.u, a.v, a.p = 16, 32, 48                      # fields but no output: rejected before anything touches the pointers
    assert h.dn_stokes_apply(C.byref(m), C.byref(a), None) == -1
    a.out[0] = 64
    a.in_num = 80                                   # in_num without in_den
    assert h.dn_stokes_apply(C.byref(m), C.byref(a), None) == -1
    a.in_num = None
    a.mask_is_u8[1] = 2
    assert h.dn_stokes_apply(C.byref(m), C.byref(a), None) == -1
    a.mask_is_u8[1] = 0
    a.bc_field[2] = 96                              # a value field without its mask
    assert h.dn_stokes_apply(C.byref(m), C.byref(a), None) == -1
    a.bc_field[2] = None
    a.norms = 112                                   # a reduction without a workspace
    assert h.dn_stokes_apply(C.byref(m), C.byref(a), None) == -3
    m.degree = 2
    assert h.dn_stokes_apply(C.byref(m), C.byref(a), None) == -2
    m.degree, m.nsd = 1, 3
    assert h.dn_stokes_apply(C.byref(m), C.byref(a), None) == -2


def test_stokes_ops_refuse_cpu_tensors_and_unsupported_meshes():
    import torch
    from diffnet_amd import DiffNet2DFEM, ops
    from diffnet_amd._lib import DiffNetHipError
    m = DiffNet2DFEM(None, domain_size=9)
    u = torch.zeros((1, 1, 9, 9))
    with pytest.raises(DiffNetHipError):
        ops.stokes_apply(m.geom, u, u, u)
    m2 = DiffNet2DFEM(None, domain_size=9, fem_basis_deg=2)
    with pytest.raises(DiffNetHipError):
        ops.stokes_apply(m2.geom, u, u, u)


# ---------------------------------------------------------------------------------------------
# float64 restatement of the operator (include/diffnet_hip.h, dn_stokes_args)
# ---------------------------------------------------------------------------------------------
def q1_tables(ngp):
    x, w = np.polynomial.legendre.leggauss(ngp)
    N = np.stack([(1 - x) / 2, (1 + x) / 2], 1)          # [ig][a]
    dN = np.stack([-0.5 * np.ones_like(x), 0.5 * np.ones_like(x)], 1)
    return N, dN, w


def stokes_np(u, v, p, masks, vals, f1, f2, visco, pspg, J, hx, hy, ngp, *, scale=False, dtype=np.float64, tables=None):
    """u, v, p, masks[k], vals[k]: (ny, nx); f1, f2: (G, nely, nelx), g = jg * ngp + ig.  Returns (R1, R2, R3), float64.
    dtype: the same statements in that type, with tables, constants and inputs cast once at entry; tables: the 1-D (N, dN, w) to use in
    place of q1_tables(ngp); scale: also returns (S1, S2, S3), S_k the sum of |w_g t| over the placed terms that make up the node's value
    (0 on the Dirichlet nodes of field k, whose value is no sum)."""
    dt = np.dtype(dtype).type
    c = lambda x: np.asarray(x, dtype=dt)                                  # noqa: E731
    N, dN, w = (c(t) for t in (q1_tables(ngp) if tables is None else tables))
    u, v, p, f1, f2 = (c(x) for x in (u, v, p, f1, f2))
    vals = [c(x) for x in vals]
    visco, pspg, J, sx, sy = dt(visco), dt(pspg), dt(J), dt(2) / dt(hx), dt(2) / dt(hy)
    ny, nx = u.shape
    fld = [np.where(m, val, t) if m is not None else t for t, m, val in zip((u, v, p), masks, vals)]
    R = [np.zeros((ny, nx), dtype=dt) for _ in range(3)]
    S = [np.zeros((ny, nx), dtype=dt) for _ in range(3)]
    for jg in range(ngp):
        for ig in range(ngp):
            g, wg = jg * ngp + ig, J * w[ig] * w[jg]
            # basis of local node (ly, lx) at the point, its x / y derivatives
            Na = {(ly, lx): N[ig, lx] * N[jg, ly] for ly in (0, 1) for lx in (0, 1)}
            Nxa = {(ly, lx): dN[ig, lx] * sx * N[jg, ly] for ly in (0, 1) for lx in (0, 1)}
            Nya = {(ly, lx): N[ig, lx] * dN[jg, ly] * sy for ly in (0, 1) for lx in (0, 1)}

            def at(t, tab):
                return sum(tab[ly, lx] * t[ly:ny - 1 + ly, lx:nx - 1 + lx] for ly in (0, 1) for lx in (0, 1))

            ux, uy, vx, vy = at(fld[0], Nxa), at(fld[0], Nya), at(fld[1], Nxa), at(fld[1], Nya)
            pg, px, py = at(fld[2], Na), at(fld[2], Nxa), at(fld[2], Nya)
            for ly in (0, 1):
                for lx in (0, 1):
                    a = (ly, lx)
                    sl = (slice(ly, ny - 1 + ly), slice(lx, nx - 1 + lx))
                    terms = (wg * (visco * (Nxa[a] * ux + Nya[a] * uy) - Nxa[a] * pg - Na[a] * f1[g]),
                             wg * (visco * (Nxa[a] * vx + Nya[a] * vy) - Nya[a] * pg - Na[a] * f2[g]),
                             wg * (Na[a] * (ux + vy) + pspg * (Nxa[a] * px + Nya[a] * py)))
                    for k, t in enumerate(terms):
                        R[k][sl] += t
                        S[k][sl] += np.abs(t)
    R = tuple(np.where(m, val, r) if m is not None else r for r, m, val in zip(R, masks, vals))
    assert all(r.dtype == dt for r in R), [r.dtype for r in R]                 # numpy promotes silently
    if not scale:
        return R
    return R, tuple(np.where(m, dt(0), s) if m is not None else s for s, m in zip(S, masks))


def fixture_case(z):
    kw = eval(str(z["kwargs"]))
    sizes = kw.get("domain_sizes", (kw["domain_size"], kw["domain_size"]))[:2]
    lengths = kw.get("domain_lengths", (kw.get("domain_length", 1.0),) * 2)[:2]
    hx, hy = lengths[0] / (sizes[0] - 1), lengths[1] / (sizes[1] - 1)
    ngp = kw.get("ngp_1d", 2)
    inp = z["inputs"].astype(np.float64)
    masks = [inp[0, 2 + k] >= 0.5 for k in range(3)]
    vals = [z[n].astype(np.float64) for n in ("u_bc", "v_bc", "p_bc")]
    f1, f2 = (z[n].astype(np.float64) for n in ("f1", "f2"))
    return dict(masks=masks, vals=vals, f1=f1, f2=f2, visco=float(z["visco"]), pspg=float(z["pspg"]), J=float(z["wscale"]),
                hx=hx, hy=hy, ngp=ngp)


@pytest.mark.parametrize("name", FIXTURES)
def test_stokes_fixtures_agree_with_float64_restatement(name):
    z = np.load(os.path.join(GOLDEN, name))
    c = fixture_case(z)
    fields = [z[n][0, 0].astype(np.float64) for n in ("u", "v", "p")]
    R = stokes_np(*fields, **c)
    for k in range(3):
        ref = z[f"R{k + 1}"][0, 0]
        np.testing.assert_allclose(R[k], ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max(), err_msg=f"R{k + 1}")
        np.testing.assert_allclose(np.linalg.norm(R[k]), z["norms"][k], rtol=1e-5)
    # the gradient of ||R_k|| is J_R^T (R_k / ||R_k|| in slot k): the transpose launch's formula, S J_R S applied to that cotangent
    lin = dict(c, vals=[0.0, 0.0, 0.0], f1=np.zeros_like(c["f1"]), f2=np.zeros_like(c["f2"]))
    for k in range(3):
        cot = [np.zeros_like(fields[0]) for _ in range(3)]
        cot[k] = R[k] / np.linalg.norm(R[k])
        cot[2] = -cot[2]
        g = list(stokes_np(*cot, **lin))
        g[2] = -g[2]
        ref = z[f"grad_norm{k + 1}"][:, 0, 0]
        for q in range(3):
            np.testing.assert_allclose(g[q], ref[q], rtol=1e-4, atol=1e-4 * np.abs(ref).max(), err_msg=f"grad of ||R{k + 1}|| wrt field {q}")


@pytest.mark.parametrize("ngp", [2, 3])
def test_stokes_jacobian_transpose_is_the_sign_flipped_jacobian(ngp):
    n = 6
    rs = np.random.default_rng(5)
    masks = [rs.random((n, n)) < 0.3 for _ in range(3)]
    zero = np.zeros(((ngp * ngp), n - 1, n - 1))
    c = dict(masks=masks, vals=[0.0, 0.0, 0.0], f1=zero, f2=zero, visco=0.7, pspg=0.05, J=0.04, hx=0.2, hy=0.25, ngp=ngp)
    nn = n * n
    Jm = np.zeros((3 * nn, 3 * nn))
    for col in range(3 * nn):
        x = np.zeros(3 * nn)
        x[col] = 1.0
        Jm[:, col] = np.concatenate([r.ravel() for r in stokes_np(*x.reshape(3, n, n), **c)])
    S = np.diag(np.concatenate([np.ones(2 * nn), -np.ones(nn)]))
    assert np.linalg.norm(Jm - Jm.T) > 1e-2 * np.linalg.norm(Jm)            # not symmetric ...
    assert np.linalg.norm(Jm.T - S @ Jm @ S) < 1e-12 * np.linalg.norm(Jm)   # ... but S-symmetric
