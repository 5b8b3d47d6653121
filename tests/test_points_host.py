"""CPU checks of the fused point-cloud terms (dn_points_apply, csrc/point_terms.hip; diffnet_amd/points.py): the C ABI and its ctypes
binding agree and the library validates its arguments before any launch; the reference fixtures (tests/golden/point_terms_*.npz, written
by tools/gen_golden_point_terms.py from the two point-cloud Poisson scripts' own loss bodies) agree with the float64 numpy restatement
tests/points_ref.py; `PointPlan` classifies, clamps, rejects and sorts as documented; and the composed torch route equals the
restatement in float64, passes gradcheck and is exact on linear fields."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import points_ref as pr
from conftest import GOLDEN

FIXTURES = ["point_terms_disk_n9.npz", "point_terms_immersed_n9.npz"]
KINDS = ("none", "dot", "match")


def geometry(nodes_xyz, deg=1):
    from diffnet_amd.fem import FemGeometry
    from diffnet_amd.tables import gauss_rule
    ngp = 2 if deg == 1 else 3
    gx, gw = gauss_rule(ngp)
    return FemGeometry(len(nodes_xyz), nodes_xyz, tuple(deg / (n - 1) for n in nodes_xyz), deg, ngp, gx, gw)


def cloud(geom, P, seed, B=1, dtype=torch.float64, faces=True):
    """(B, P, nsd) points in the physical column order (x, y[, z]): seeded interior points, then -- where they fit -- points on the
    domain's faces and corners and on interior element faces"""
    g = torch.Generator().manual_seed(seed)
    nsd = geom.nsd
    L = torch.tensor([geom.hs[d] * geom.nel[d] for d in range(nsd)], dtype=torch.float64)
    pts = torch.rand((B, P, nsd), generator=g, dtype=torch.float64) * L
    if faces:
        special = [[0.0] * nsd, [float(v) for v in L], [0.0] + [float(v) for v in L[1:]]]
        special += [[geom.hs[d] * min(1 + d, geom.nel[d] - 1) if j == d else 0.37 * float(L[j]) for j in range(nsd)] for d in range(nsd)]       # interior element faces
        special += [[float(L[d]) if j == d else 0.61 * float(L[j]) for j in range(nsd)] for d in range(nsd)]                # far faces
        for k, s in enumerate(special[:max(0, P - 1)]):
            pts[:, k] = torch.tensor(s, dtype=torch.float64)
    return pts.to(dtype)


def plan_arrays(plan):
    """the plan's sorted points as points_ref takes them: sample b (T), element per mesh axis (T, nsd), xi (T, nsd) float64"""
    geom = plan.geom
    e = plan.elem.cpu().numpy().astype(np.int64)
    ed = []
    for d in range(geom.nsd):
        ed.append(e % geom.nel[d])
        e = e // geom.nel[d]
    b = np.repeat(np.arange(plan.B), plan.P)
    return b, np.stack(ed, 1), plan.xi.cpu().numpy().astype(np.float64).T


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_points_abi_header_and_binding_agree():
    from diffnet_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "..", "include", "diffnet_hip.h")).read()
    for s in ("dn_points_workspace_bytes", "dn_points_apply"):
        assert hasattr(h, s) and s in _lib.SYMBOLS and s + "(const dn_mesh *mesh" in header, s
    assert h.dn_abi_version() == _lib.ABI_VERSION == 10
    assert "#define DN_ABI_VERSION 10" in header
    assert "point_terms.hip" in build.SOURCES
    for name, val in (("DN_POINTS_NONE", _lib.POINTS_NONE), ("DN_POINTS_DOT", _lib.POINTS_DOT), ("DN_POINTS_MATCH", _lib.POINTS_MATCH)):
        assert f"#define {name} {val}" in header
    # the struct of the binding has the members of the header's, in its order
    body = header.split("typedef struct dn_points_args {")[1].split("} dn_points_args;")[0]
    names = [ln.split(";")[0].replace("*", " ").replace("[3]", "").split()[-1] for ln in body.splitlines() if ";" in ln and "," not in ln.split(";")[0]]
    multi = [n.strip() for ln in body.splitlines() if ";" in ln and "," in ln.split(";")[0] for n in ln.split(";")[0].replace("float", "").split(",")]
    assert set(names + multi) == {f[0] for f in _lib.DnPointsArgs._fields_}
    assert h.dn_points_workspace_bytes(C.byref(geometry((9, 7)).mesh_struct(2))) == 4160 + 16 * 1024
    assert h.dn_points_workspace_bytes(C.byref(geometry((5, 6, 7)).mesh_struct(1))) == 4160 + 16 * 1024


def test_points_argument_validation_without_a_gpu():
    from diffnet_amd import _lib
    h = _lib.lib()
    m = geometry((9, 7)).mesh_struct(2)

    def args(**kw):
        # every pointer is a small odd number: a check that came after a launch or a dereference would not return
        a = _lib.DnPointsArgs()
        a.u, a.elem, a.xi, a.offsets, a.npts = 17, 33, 65, 129, 5
        a.dscale[:] = (1.0, 1.0, 1.0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda mesh, a: h.dn_points_apply(C.byref(mesh), C.byref(a), None)       # noqa: E731
    assert h.dn_points_apply(None, None, None) == -1
    assert h.dn_points_apply(C.byref(m), None, None) == -1
    assert h.dn_points_apply(None, C.byref(args(values=257)), None) == -1
    assert h.dn_points_workspace_bytes(None) == -1
    assert call(m, args()) == -1                                           # nothing to compute
    assert call(m, args(accumulate=1)) == -1                               # accumulate without grad
    assert call(m, args(accumulate=1, values=257)) == -1
    assert call(m, args(values=257, u=None)) == -1                         # null pointers
    assert call(m, args(values=257, elem=None)) == -1
    assert call(m, args(pgrads=257, xi=None)) == -1
    assert call(m, args(grad=257, cot=None)) == -1
    assert call(m, args(grad=257, cot=513, offsets=None)) == -1
    assert call(m, args(values=257, npts=-1)) == -1                        # sizes
    assert call(m, args(values=257, npts=2 ** 30)) == -1                   # B npts >= 2^31
    assert call(m, args(values=257, kind=3)) == -1                         # unknown kind
    assert call(m, args(values=257, kind=-1)) == -1
    assert call(m, args(values=257, penalty=2, cot=513)) == -1             # flags outside {0, 1}
    assert call(m, args(grad=257, cot=513, accumulate=2)) == -1
    assert call(m, args(penalty=1)) == -1                                  # a penalty nobody reads
    assert call(m, args(values=257, sums=1025)) == -1                      # sums without the penalty
    assert call(m, args(penalty=1, cot=513, kind=_lib.POINTS_DOT)) == -1   # a normals term without normals
    assert call(m, args(penalty=1, cot=513, kind=_lib.POINTS_MATCH)) == -1
    assert call(m, args(penalty=1, sums=1025)) == -3                       # sums without a workspace ...
    assert call(m, args(penalty=1, sums=1025, workspace=2049, workspace_bytes=64)) == -3       # ... or with one that is too small
    assert call(m, args(penalty=1, sums=1025, workspace=2049, workspace_bytes=h.dn_points_workspace_bytes(C.byref(m)) - 1)) == -3
    for field, bad, code in (("degree", 2, -2), ("degree", 3, -2), ("degree", 0, -1), ("nsd", 1, -1), ("nsd", 4, -1), ("nx", 1, -1), ("ny", 0, -1),
                             ("nz", 2, -1), ("batch", 0, -1), ("batch", 65536, -1)):
        mm = geometry((9, 7)).mesh_struct(3)
        mm = type(mm).from_buffer_copy(mm)
        setattr(mm, field, bad)
        assert call(mm, args(values=257)) == code, field
        assert h.dn_points_workspace_bytes(C.byref(mm)) == code, field
    m3 = type(m).from_buffer_copy(geometry((5, 6, 7)).mesh_struct(1))
    m3.nz = 1
    assert call(m3, args(values=257)) == -1
    m3.nx, m3.ny, m3.nz = 1024, 1024, 1024                                 # 2^30 nodes per sample
    assert call(m3, args(values=257)) == -2


# ---------------------------------------------------------------------------------------------
# the reference fixtures against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", FIXTURES)
def test_points_ref_reproduces_the_reference_differences(fixture):
    z = np.load(os.path.join(GOLDEN, fixture))
    n = int(z["n"])
    h = 1.0 / (n - 1)
    u = z["u"][0]                                                          # (1, n, n)
    tol = 1e-12 * (abs(float(z["loss_a"])) + abs(float(z["loss_a1"])))

    def term(pc, field, swap):
        # the scripts' u[b, 0, nidx, nidy]: x indexes rows, i.e. point column 0 runs along mesh axis 1
        e, xi = pr.classify(pc[:, ::-1] if swap else pc, (h, h), (n - 1, n - 1))
        lv, ln, grad = pr.loss_and_grad(field, np.zeros(len(pc), dtype=np.int64), e, xi, (1.0, 1.0), 1.0, None, "none")
        return lv + ln, grad

    dl, dg = float(z["loss_a"]) - float(z["loss_a1"]), (z["grad_a"] - z["grad_a1"])[0]
    la, ga = term(z["cloud_a"], u, True)
    l1, g1 = term(z["cloud_a1"], u, True)
    assert abs((la - l1) - dl) <= tol
    assert np.abs((ga - g1) - dg).max() <= tol
    # the same with the physical order on the transposed field
    ut = np.ascontiguousarray(np.swapaxes(u, 1, 2))
    la, ga = term(z["cloud_a"], ut, False)
    l1, g1 = term(z["cloud_a1"], ut, False)
    assert abs((la - l1) - dl) <= tol
    assert np.abs(np.swapaxes(ga - g1, 1, 2) - dg).max() <= tol
    # the fixture holds what the issue asks of it: a point on an interior element boundary, one at x = 0, none at x = L
    a = z["cloud_a"]
    assert np.any(a[:, 0] == 3 * h) and np.any(a[:, 0] == 0.0) and a.max() < 1.0 and len(a) == 40 and len(z["cloud_a1"]) == 1


@pytest.mark.parametrize("fixture", FIXTURES)
def test_point_loss_axes_transposed_reproduces_the_reference_differences(fixture):
    """the public function on the composed route (CPU, float64): axes="transposed" on u equals the physical order on u^T, and both
    equal the reference's differences to the rounding of the plan's float32 local coordinates"""
    from diffnet_amd import points as P
    z = np.load(os.path.join(GOLDEN, fixture))
    n = int(z["n"])
    geom = geometry((n, n))
    out = {}
    for axes, field in (("transposed", z["u"]), (None, np.ascontiguousarray(np.swapaxes(z["u"], 2, 3)))):
        res = []
        for name in ("cloud_a", "cloud_a1"):
            u = torch.from_numpy(field).requires_grad_(True)
            plan = P.PointPlan(geom, torch.from_numpy(z[name]), axes=axes)
            loss = P.point_loss(geom, u, plan, target=1.0)
            loss.backward()
            res.append((float(loss.detach()), u.grad.numpy()[0]))
        out[axes] = (res[0][0] - res[1][0], res[0][1] - res[1][1])
    dl, dg = float(z["loss_a"]) - float(z["loss_a1"]), (z["grad_a"] - z["grad_a1"])[0]
    assert abs(out["transposed"][0] - out[None][0]) <= 1e-12 * abs(dl)
    assert np.abs(out["transposed"][1] - np.swapaxes(out[None][1], 1, 2)).max() <= 1e-12 * np.abs(dg).max()
    # xi is rounded to float32 (2^-24 relative, |xi| <= 1) and enters each of the 40 terms linearly: 40 x 2^-24 x the terms' scale
    assert abs(out["transposed"][0] - dl) <= 40 * 2.0 ** -24 * (abs(float(z["loss_a"])) + abs(float(z["loss_a1"])))
    assert np.abs(out["transposed"][1] - dg).max() <= 40 * 2.0 ** -24 * np.abs(dg).max()


# ---------------------------------------------------------------------------------------------
# PointPlan
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nodes,dtype", [((9, 7), torch.float64), ((9, 7), torch.float32), ((5, 6, 7), torch.float64), ((5, 6, 7), torch.float32)])
def test_plan_classifies_like_the_restatement(nodes, dtype):
    from diffnet_amd import points as P
    geom = geometry(nodes)
    pts = cloud(geom, 65, 5, B=2, dtype=dtype)
    plan = P.PointPlan(geom, pts)
    npd = np.float64 if dtype == torch.float64 else np.float32
    b, e, xi = plan_arrays(plan)
    order = plan.order.numpy()
    flat = pts.reshape(-1, geom.nsd).numpy()
    er, xr = pr.classify(flat, geom.hs, geom.nel, npd)
    assert np.array_equal(e, er[order])
    assert np.array_equal(plan.xi.numpy().T, xr[order].astype(np.float32))
    # sorted by (sample, element), stably; the offsets are the CSR of the sorted ids; the permutation round-trips
    key = b * geom.nelem_total + pr.flat_element(e, geom.nel)
    assert np.all(np.diff(key) >= 0)
    assert np.array_equal(order, np.argsort(np.repeat(np.arange(2), 65) * geom.nelem_total + pr.flat_element(er, geom.nel), kind="stable"))
    off = plan.offsets.numpy()
    assert off.dtype == np.int32 and len(off) == 2 * geom.nelem_total + 1 and off[0] == 0 and off[-1] == plan.T
    assert np.array_equal(np.diff(off), np.bincount(key, minlength=2 * geom.nelem_total))
    assert plan.elem.dtype == torch.int32 and plan.xi.dtype == torch.float32 and plan.xi.shape == (geom.nsd, plan.T)
    t = torch.arange(plan.T, dtype=torch.float64).reshape(2, 65)
    assert torch.equal(plan.unsort(plan.sort(t)), t)
    v = pts.double()
    assert torch.equal(plan.unsort(plan.sort(v, vector=True), vector=True), v)
    assert torch.equal(plan.inv[plan.order], torch.arange(plan.T))


def test_plan_far_face_clamps_to_the_last_element():
    from diffnet_amd import points as P
    for nodes in ((9, 7), (5, 6, 7), (50, 4)):
        geom = geometry(nodes)
        L = [geom.hs[d] * geom.nel[d] for d in range(geom.nsd)]
        for dtype in (torch.float32, torch.float64):
            pts = torch.tensor([[1.0] * geom.nsd, [0.0] * geom.nsd], dtype=dtype)
            plan = P.PointPlan(geom, pts)
            b, e, xi = plan_arrays(plan)
            assert np.array_equal(e[plan.inv.numpy()], [[n - 1 for n in geom.nel], [0] * geom.nsd])
            assert np.array_equal(xi[plan.inv.numpy()], [[1.0] * geom.nsd, [-1.0] * geom.nsd])
        assert all(abs(v - 1.0) < 1e-15 for v in L)


def test_plan_rejects_points_outside_and_non_finite_points():
    from diffnet_amd import points as P
    geom = geometry((9, 7))
    good = cloud(geom, 9, 1)
    for col in (0, 1):
        for bad in (-1e-9, 1.0 + 1e-6, float("nan"), float("inf"), -float("inf")):
            pts = good.clone()
            pts[0, 4, col] = bad
            with pytest.raises(ValueError):
                P.PointPlan(geom, pts)
    with pytest.raises(ValueError):
        P.PointPlan(geom, good[..., :1])
    with pytest.raises(ValueError):
        P.PointPlan(geom, good, axes=(0, 0))
    with pytest.raises(ValueError):
        P.PointPlan(geom, good, classify="nearest")
    with pytest.raises(TypeError):
        P.PointPlan(geom, good.long())


def test_plan_shared_cloud_equals_the_explicit_batch_and_axes():
    from diffnet_amd import points as P
    geom = geometry((9, 7))
    pts = cloud(geom, 17, 2)[0]
    shared, explicit = P.PointPlan(geom, pts, batch=3), P.PointPlan(geom, pts[None].expand(3, -1, -1).contiguous())
    for name in ("elem", "xi", "order", "inv", "offsets"):
        assert torch.equal(getattr(shared, name), getattr(explicit, name)), name
    # "transposed": column c indexes spatial axis c -- the physical plan of the swapped columns
    tr, ph = P.PointPlan(geom, pts.flip(-1), axes="transposed"), P.PointPlan(geom, pts)
    for name in ("elem", "xi", "order", "offsets"):
        assert torch.equal(getattr(tr, name), getattr(ph, name)), name
    assert tr.cols == (1, 0) and ph.cols == (0, 1)
    # an empty cloud is a valid plan
    empty = P.PointPlan(geom, pts[:0], batch=2)
    assert empty.T == 0 and empty.offsets.shape == (2 * geom.nelem_total + 1,) and int(empty.offsets.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------
# the composed route on the CPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nodes", [(9, 7), (5, 6, 7)])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dscale", [None, "physical"])
def test_composed_matches_the_restatement_in_float64(nodes, kind, dscale):
    from diffnet_amd import points as P
    geom = geometry(nodes)
    B, Pn = 2, 33
    g = torch.Generator().manual_seed(11)
    u = torch.randn((B, 1, *geom.node_shape), generator=g, dtype=torch.float64)
    pts = cloud(geom, Pn, 3, B=B)
    normals = torch.randn((B, Pn, geom.nsd), generator=g, dtype=torch.float64)
    target = torch.randn((B, Pn), generator=g, dtype=torch.float64)
    plan = P.PointPlan(geom, pts)
    b, e, xi = plan_arrays(plan)
    ds = plan.dscale(dscale)
    assert ds == ((1.0,) * geom.nsd if dscale is None else tuple(2.0 / h for h in geom.hs))
    order = plan.order.numpy()
    ts, ns = target.reshape(-1).numpy()[order], normals.reshape(-1, geom.nsd).numpy()[order]
    lv, ln, grad = pr.loss_and_grad(u.numpy()[:, 0], b, e, xi, ds, ts, ns, kind, 0.7, 1.3)
    ur = u.clone().requires_grad_(True)
    tv, tn = P.point_terms_composed(geom, ur, plan, target, normals, kind, 0.7, 1.3, dscale, terms=True)
    (tv + tn).backward()
    assert abs(float(tv.detach()) - lv) <= 1e-12 * abs(lv) and abs(float(tn.detach()) - ln) <= 1e-12 * max(abs(ln), abs(lv))
    assert np.abs(ur.grad.numpy()[:, 0] - grad).max() <= 1e-12 * np.abs(grad).max()
    # the public functions on a CPU tensor take this route, and loss_and_grad accumulates
    loss = P.point_loss(geom, u, plan, target, normals, kind, 0.7, 1.3, dscale)
    assert abs(float(loss) - (lv + ln)) <= 1e-12 * abs(lv + ln)
    buf = torch.ones_like(u)
    l2, g2 = P.point_loss_and_grad(geom, u, plan, target, normals, kind, 0.7, 1.3, dscale, grad_out=buf, accumulate=True)
    assert g2 is buf and abs(float(l2) - (lv + ln)) <= 1e-12 * abs(lv + ln)
    assert np.abs(buf.numpy()[:, 0] - 1.0 - grad).max() <= 1e-12 * np.abs(grad).max()
    vals, grads = P.eval_at_points(geom, u, plan, dscale)
    rv, rg, _, _ = pr.interpolate(u.numpy()[:, 0], b, e, xi, ds)
    inv = plan.inv.numpy()
    assert vals.shape == (B, Pn) and grads.shape == (B, Pn, geom.nsd)
    assert np.abs(vals.reshape(-1).numpy() - rv[inv]).max() <= 1e-12 * np.abs(rv).max()
    assert np.abs(grads.reshape(-1, geom.nsd).numpy() - rg[inv]).max() <= 1e-12 * np.abs(rg).max()


@pytest.mark.parametrize("nodes", [(5, 4), (4, 3, 5)])
def test_composed_gradcheck(nodes):
    from diffnet_amd import points as P
    geom = geometry(nodes)
    g = torch.Generator().manual_seed(2)
    u = torch.randn((2, 1, *geom.node_shape), generator=g, dtype=torch.float64, requires_grad=True)
    pts = cloud(geom, 11, 9, B=2)
    normals = torch.randn((2, 11, geom.nsd), generator=g, dtype=torch.float64, requires_grad=True)
    target = torch.randn((2, 11), generator=g, dtype=torch.float64, requires_grad=True)
    plan = P.PointPlan(geom, pts)
    for kind in KINDS:
        assert torch.autograd.gradcheck(lambda a, t, n: P.point_loss(geom, a, plan, t, n, kind, 0.5, 2.0, "physical"), (u, target, normals))
    assert torch.autograd.gradcheck(lambda a: P.eval_at_points(geom, a, plan, "physical"), (u,))


@pytest.mark.parametrize("nodes,deg", [((9, 7), 1), ((5, 6, 7), 1), ((9, 7), 2), ((7, 7, 4), 3)])
def test_linear_fields_are_reproduced_exactly(nodes, deg):
    """u = a + b . x: the values and the physical gradients (dscale = 2 / h) are exact to rounding at every point, points on element
    faces and on the domain's faces included -- on Q2 / Q3 meshes too, where the composed route is the only one"""
    from diffnet_amd import points as P
    geom = geometry(nodes, deg)
    nsd = geom.nsd
    coef = [0.3, -1.7, 0.9, 2.2][:nsd + 1]
    axes = [torch.linspace(0.0, 1.0, n, dtype=torch.float64) for n in geom.sizes]            # x, y[, z]
    u = torch.full(geom.node_shape, coef[0], dtype=torch.float64)
    for d in range(nsd):
        shape = [1] * nsd
        shape[nsd - 1 - d] = -1
        u = u + coef[1 + d] * axes[d].reshape(shape)
    pts = cloud(geom, 40, 4)
    plan = P.PointPlan(geom, pts)
    vals, grads = P.eval_at_points(geom, u[None, None], plan, "physical")
    exact = coef[0] + sum(coef[1 + d] * pts[..., d] for d in range(nsd))
    # xi carries a float32 rounding of a number in [-1, 1]: 2^-24 x (h / 2) x |b| in the value; the gradient does not depend on xi
    assert float((vals - exact).abs().max()) <= 2.0 ** -24 * sum(abs(c) for c in coef[1:]) * 0.5 * max(geom.hs) + 1e-14
    for d in range(nsd):
        assert float((grads[..., d] - coef[1 + d]).abs().max()) <= 1e-12
