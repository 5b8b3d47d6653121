"""The fused point-cloud terms (csrc/point_terms.hip: dn_points_apply; ops.points_apply; diffnet_amd/points.py) on the GPU against the
float64 restatement tests/points_ref.py, built from the plan's own float32 local coordinates and the same float32 field.

Meshes 9 x 7 nodes (nx != ny) and 5 x 6 x 7 nodes, B = 2 with clouds that differ per sample; 1, 63, 64, 65, 257 and 1025 points per
sample (waves, workgroups, several workgroups in the reduction), 2 x 140 000 points (more than the 1024 x 256 points one pass of the
forward grid holds), no points at all; points on every face and corner of the domain and on interior element faces, 70 points in one
element (the inner loop of the adjoint) and, at the small counts, mostly empty elements.

Every comparison is a derived bound, not a chosen tolerance: u = 2^-24, gamma(k) = k u / (1 - k u), k the number of roundings on the
longest path of the kernel's own chain (csrc/point_terms.hip), errors relative to the sum of the absolute values of the terms:
  weights    N0 = 0.5 fl(1 - xi), N1 = 0.5 fl(1 + xi)                       1 each (the halving is exact)
  value      per axis  fma(N1, hi, fl(N0 lo)): weight 1 + product 1 + fma 1 = 3 per axis            k = 6 in 2-D, 9 in 3-D
  derivative on its own axis 0.5 fl(hi - lo): 1;  the other axes 3 each;  the scale s_d: 1          k = 1 + 3 + 1 = 5 in 2-D, 1 + 6 + 1 = 8 in 3-D
  cot        c0 = fl(2 w fl(u_p - t)): 2, relative to |c0|;  match: c_d = fl(2 w fl(g_d - n_d)): 2;
             dot: the dot product nsd (first product, then fmas), "- 1" 1, relative to sum |g_d n_d| + 1, then two products: nsd + 3
  sums       the squares of the float32 residuals are summed in float64: the residuals' own roundings (1, or nsd + 1 as above) enter as
             2 |r| e + e^2, the accumulation with (terms + 10) 2^-53
  adjoint    N_a = fl(fl(wx wy) wz): 3 weights + 2 products = 5 (2-D: 3);  s_d d_d N_a: at most 4 (2);  one fma per term into one
             accumulator: a term passes at most the M = (1 + nsd) x (points of the node's adjacent elements) roundings of the chain;
             gs = fl(gscale gscale_dev) and fl(gs acc): 2                    k = 5 + M + 2 in 3-D, 3 + M + 2 in 2-D
The composed torch route in float32 has its own chain -- products of the weights (3 | 5), the product with u (1), a sum of 4 | 8 terms
(3 | 7): 7 | 13 for a value, 6 | 12 for a derivative -- and the two routes are compared under the sum of both bounds, propagated
through the penalty (2 |r| e + e^2 per residual) and the adjoint.

Largest |got - ref| / bound per quantity on the MI355X (each test prints its own; run with -s): RATIOS_OBSERVED below.
"""
import numpy as np
import pytest
import torch

import points_ref as pr
from test_gpu_parity import dev
from test_points_host import cloud, geometry, plan_arrays

pytestmark = pytest.mark.gpu

RATIOS_OBSERVED = ("values 0.53, derivatives 0.64, cot 0.97, sums 0.54, adjoint 0.31, fused vs composed 0.24 "
                   "(values, derivatives and cot: the largest of the 280 000 points of the two-pass case; 0.36, 0.47 and 0.82 at the other counts)")

U = 2.0 ** -24
KV, KD, KA = {2: 6, 3: 9}, {2: 5, 3: 8}, {2: 3, 3: 5}
KV_C, KD_C = {2: 7, 3: 13}, {2: 6, 3: 12}
MESHES = {2: (9, 7), 3: (5, 6, 7)}
COUNTS = (1, 63, 64, 65, 257, 1025)
KINDS = ("none", "dot", "match")
RATIOS = {}


def gam(k):
    return k * U / (1.0 - k * U)


def check(what, case, err, bound):
    """err <= bound everywhere; where the bound is 0 the error must be 0"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.all(err[bound == 0.0] == 0.0), f"{what} {case}: an error where the bound is zero"
    r = float(np.max(err[bound > 0.0] / bound[bound > 0.0])) if np.any(bound > 0.0) else 0.0
    RATIOS[what] = max(RATIOS.get(what, 0.0), r)
    print(f"points-ratio {what} {case}: {r:.3g} (max so far {RATIOS[what]:.3g})")
    assert r <= 1.0, f"{what} {case}: |got - ref| is {r:.3g} x the bound"


def problem(nsd, P, seed=0, B=2, crowd=None):
    """geometry, field, cloud (physical column order), normals, targets: float32 on the GPU"""
    geom = geometry(MESHES[nsd])
    g = torch.Generator().manual_seed(100 * nsd + P % 97 + seed)
    u = torch.randn((B, 1, *geom.node_shape), generator=g).float()
    pts = cloud(geom, P, 7 + seed, B=B, dtype=torch.float32)
    if (crowd is None and P >= 257) or crowd:                     # 70 points in one interior element of sample 0, a different one in sample 1
        for b in range(B):
            lo = torch.tensor([geom.hs[d] * (1 + b) for d in range(nsd)])
            pts[b, 20:90] = lo + torch.rand((70, nsd), generator=g) * torch.tensor(geom.hs[:nsd]) * 0.98 + 0.01 * torch.tensor(geom.hs[:nsd])
    pts[1] = pts[1].flip(0)                                       # the samples see their points in different orders
    normals = torch.nn.functional.normalize(torch.randn((B, P, nsd), generator=g), dim=-1)
    target = 0.3 * torch.randn((B, P), generator=g)
    d = dev()
    return geom, u.to(d), pts.to(d), normals.to(d), target.to(d)


def ds32(plan, dscale):
    return tuple(float(np.float32(s)) for s in plan.dscale(dscale))


def forward_and_adjoint(geom, plan, u, target, normals, kind, w_val, w_nrm, dscale, gscale=1.0, gdev=None):
    from diffnet_amd import ops
    tgt = plan.sort(target) if isinstance(target, torch.Tensor) else target
    nrm = plan.sort(normals, vector=True) if kind != "none" else None
    vals, pg, sums, cot, grad = ops.points_apply(geom, plan.B, plan.P, plan.xi, plan.elem, plan.offsets, u=u, dscale=plan.dscale(dscale), kind=kind,
                                                 penalty=True, target=tgt, normals=nrm, w_val=w_val, w_nrm=w_nrm, want_values=True,
                                                 want_pgrads=True, want_sums=True, want_cot=True, want_grad=True, gscale=gscale, gscale_dev=gdev)
    return vals, pg, sums, cot, grad, tgt, nrm


def residual_bounds(val, g, tgt, nrm, kind, ev, eg, routes=1):
    """per residual of the penalty: (its value, the bound of its error) given error bounds ev (N), eg (N, nsd) of u_p and g_d; `routes`:
    how many float32 evaluations the bound has to cover (2: the difference of two routes)"""
    nsd = g.shape[1]
    dv = val - tgt
    out = [(dv, ev + routes * U * np.abs(dv))]
    if kind == "dot":
        out.append((np.sum(g * nrm, 1) - 1.0, np.sum(np.abs(nrm) * eg, 1) + routes * gam(nsd + 1) * (np.sum(np.abs(g * nrm), 1) + 1.0)))
    elif kind == "match":
        out.append((g - nrm, eg + routes * U * np.abs(g - nrm)))
    return out


def loss_bound(r, e, w, terms):
    return abs(w) * float(np.sum(2.0 * np.abs(r) * e + e * e)) + (terms + 10) * 2.0 ** -53 * abs(w) * float(np.sum(r * r))


def cot_bounds(res, c0, c, nrm, kind, w_val, w_nrm, routes=1):
    """the residuals' bounds through c = 2 w r [n_d], plus the products' own roundings: 1 (c0, match), 2 (dot)"""
    e0 = 2.0 * abs(w_val) * res[0][1] + routes * gam(1) * np.abs(c0)
    if kind == "dot":
        return e0, 2.0 * abs(w_nrm) * np.abs(nrm) * res[1][1][:, None] + routes * gam(2) * np.abs(c)
    if kind == "match":
        return e0, 2.0 * abs(w_nrm) * res[1][1] + routes * gam(1) * np.abs(c)
    return e0, np.zeros_like(c)


def check_against_ref(case, geom, plan, u, target, normals, kind, w_val, w_nrm, dscale, gscale=1.0, gdev=None):
    nsd = geom.nsd
    w32v, w32n, gs = float(np.float32(w_val)), float(np.float32(w_nrm)), float(np.float32(gscale)) * (1.0 if gdev is None else float(gdev[0]))
    vals, pg, sums, cot, grad, tgt, nrm = forward_and_adjoint(geom, plan, u, target, normals, kind, w_val, w_nrm, dscale, gscale, gdev)
    b, e, xi = plan_arrays(plan)
    ds = ds32(plan, dscale)
    u64 = u.cpu().numpy().astype(np.float64)[:, 0]
    rv, rg, av, ag = pr.interpolate(u64, b, e, xi, ds)
    kv, kg = vals.cpu().numpy().astype(np.float64), pg.cpu().numpy().astype(np.float64).T
    check("values", case, np.abs(kv - rv), gam(KV[nsd]) * av)
    check("derivatives", case, np.abs(kg - rg), gam(KD[nsd]) * ag)
    # the penalty from the kernel's own float32 values: only the roundings after them are left
    t64 = tgt.cpu().numpy().astype(np.float64) if isinstance(tgt, torch.Tensor) else float(np.float32(tgt))
    n64 = nrm.cpu().numpy().astype(np.float64).T if nrm is not None else None
    zero_v, zero_g = np.zeros_like(kv), np.zeros_like(kg)
    res = residual_bounds(kv, kg, t64, n64, kind, zero_v, zero_g)
    lv, ln, c0, c = pr.penalty(kv, kg, t64, n64, kind, w32v, w32n)
    kc = cot.cpu().numpy().astype(np.float64)
    e0, ec = cot_bounds(res, c0, c, n64, kind, w32v, w32n)
    check("cot", case, np.abs(kc[0] - c0), e0)
    if kind != "none":
        check("cot", case + " normals", np.abs(kc[1:].T - c), ec)
    else:
        assert not kc[1:].any()
    s = sums.cpu().numpy()
    bv = loss_bound(res[0][0], res[0][1], w32v, plan.T)
    bn = loss_bound(res[1][0], res[1][1], w32n, plan.T * nsd) if kind != "none" else 0.0
    check("sums", case, [abs(s[0] - lv), abs(s[1] - ln), abs(s[2] - (lv + ln))], [bv, bn, bv + bn + 2.0 ** -52 * abs(lv + ln)])
    # the adjoint from the kernel's own cotangents
    shape = (plan.B, *geom.node_shape)
    rgrad, agrad, cnt = pr.adjoint(shape, b, e, xi, kc[0], kc[1:].T, ds, gs)
    kgrad = grad.cpu().numpy().astype(np.float64)[:, 0]
    k = KA[nsd] + (1 + nsd) * cnt + 2
    check("adjoint", case, np.abs(kgrad - rgrad), k * U / (1.0 - k * U) * agrad)
    assert not kgrad[cnt == 0].any()                              # exactly zero where no adjacent element holds a point
    return sums, cot, grad


@pytest.mark.parametrize("nsd", [2, 3])
@pytest.mark.parametrize("P", COUNTS)
def test_points_against_float64_at_every_seam(nsd, P):
    from diffnet_amd import points as pp
    geom, u, pts, normals, target = problem(nsd, P)
    plan = pp.PointPlan(geom, pts)
    if P >= 257:
        assert int(torch.diff(plan.offsets).max()) >= 70
    if P < geom.nelem_total:
        assert int((torch.diff(plan.offsets) == 0).sum()) > 0      # empty elements (fewer points than elements)
    for kind, dscale, tgt in (("dot", "physical", target), ("match", None, 0.25), ("none", None, target)):
        check_against_ref(f"{nsd}d P={P} {kind}", geom, plan, u, tgt, normals, kind, 0.7, 1.3, dscale)
    check_against_ref(f"{nsd}d P={P} dot scaled", geom, plan, u, target, normals, "dot", 0.7, 1.3, "physical", gscale=0.6,
                      gdev=torch.tensor([1.7], device=dev()))


def test_points_more_than_one_pass_of_the_forward_grid():
    from diffnet_amd import points as pp
    geom, u, pts, normals, target = problem(2, 140000, crowd=False)
    plan = pp.PointPlan(geom, pts)
    assert plan.T > 1024 * 256
    check_against_ref("2d P=140000 dot", geom, plan, u, target, normals, "dot", 1.0 / plan.T, 1.0 / plan.T, "physical")


@pytest.mark.parametrize("nsd", [2, 3])
def test_points_empty_cloud(nsd):
    from diffnet_amd import ops, points as pp
    geom, u, pts, normals, target = problem(nsd, 5)
    plan = pp.PointPlan(geom, pts[:, :0])
    assert plan.T == 0
    loss, grad = pp.point_loss_and_grad(geom, u, plan, 0.0, normals[:, :0], "dot")
    assert float(loss) == 0.0 and grad.shape == u.shape and not grad.any()
    buf = torch.randn_like(u)
    keep = buf.clone()
    loss, out = pp.point_loss_and_grad(geom, u, plan, 0.0, None, grad_out=buf, accumulate=True)
    assert out is buf and torch.equal(buf, keep) and float(loss) == 0.0
    _, _, sums, _, _ = ops.points_apply(geom, plan.B, 0, plan.xi, plan.elem, u=u, penalty=True, want_sums=True)
    assert sums.tolist() == [0.0, 0.0, 0.0]
    ur = u.clone().requires_grad_(True)
    pp.point_loss(geom, ur, plan).backward()
    assert not ur.grad.any()
    vals, grads = pp.eval_at_points(geom, u, plan)
    assert vals.shape == (2, 0) and grads.shape == (2, 0, nsd)


@pytest.mark.parametrize("nsd", [2, 3])
def test_points_bitwise(nsd):
    from diffnet_amd import points as pp
    geom, u, pts, normals, target = problem(nsd, 1025)
    plan = pp.PointPlan(geom, pts)
    args = (target, normals, "dot", 0.7, 1.3, "physical")
    l1, g1 = pp.point_loss_and_grad(geom, u, plan, *args)
    l2, g2 = pp.point_loss_and_grad(geom, u, plan, *args)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)                                    # two runs
    # each sample's points regrouped element by element in a random element order, the order within an element kept: the same
    # multiset per element in the same relative order
    gen = torch.Generator().manual_seed(3)
    nel = geom.nelem_total
    elem_of = torch.empty((plan.B, plan.P), dtype=torch.long)
    elem_of.view(-1)[plan.order.cpu()] = plan.elem.cpu().long()
    perm = torch.stack([torch.sort(torch.randperm(nel, generator=gen)[elem_of[b]], stable=True).indices for b in range(plan.B)]).to(dev())
    take = lambda t: torch.gather(t, 1, perm.reshape(plan.B, plan.P, *([1] * (t.dim() - 2))).expand(-1, -1, *t.shape[2:]))     # noqa: E731
    plan_p = pp.PointPlan(geom, take(pts))
    assert torch.equal(plan_p.xi, plan.xi) and torch.equal(plan_p.elem, plan.elem) and not torch.equal(plan_p.order, plan.order)
    l3, g3 = pp.point_loss_and_grad(geom, u, plan_p, take(target), take(normals), *args[2:])
    assert torch.equal(l1, l3) and torch.equal(g1, g3)
    # accumulate onto a known buffer: buffer + gradient, bitwise; a scaled gradient likewise
    for gscale in (1.0, 0.375, 1.7):
        _, g = pp.point_loss_and_grad(geom, u, plan, *args, gscale=gscale)
        buf = torch.randn_like(u)
        want = buf + g
        _, out = pp.point_loss_and_grad(geom, u, plan, *args, grad_out=buf, accumulate=True, gscale=gscale)
        assert out is buf and torch.equal(buf, want)
    buf = torch.full_like(u, 7.0)
    _, out = pp.point_loss_and_grad(geom, u, plan, *args, grad_out=buf)                   # overwrite, not add
    assert torch.equal(out, g1)
    # a node none of whose adjacent elements holds a point: exactly zero, and untouched (its -0 kept) under accumulate
    plan_s = pp.PointPlan(geom, pts[:, :3])
    _, gs = pp.point_loss_and_grad(geom, u, plan_s, target[:, :3], normals[:, :3], *args[2:])
    b, e, xi = plan_arrays(plan_s)
    _, _, cnt = pr.adjoint((plan_s.B, *geom.node_shape), b, e, xi, np.zeros(plan_s.T), np.zeros((plan_s.T, nsd)), (1.0,) * nsd)
    free = torch.from_numpy(cnt == 0)[:, None].to(dev())
    assert int(free.sum()) > 0 and not gs[free].any()
    buf = torch.full_like(u, -0.0)
    pp.point_loss_and_grad(geom, u, plan_s, target[:, :3], normals[:, :3], *args[2:], grad_out=buf, accumulate=True)
    assert torch.equal(torch.signbit(buf[free]), torch.ones_like(buf[free], dtype=torch.bool))


@pytest.mark.parametrize("nsd", [2, 3])
def test_points_autograd(nsd):
    from diffnet_amd import points as pp
    geom, u, pts, normals, target = problem(nsd, 257)
    plan = pp.PointPlan(geom, pts)
    args = (target, normals, "match", 0.7, 1.3, "physical")
    loss0, g0 = pp.point_loss_and_grad(geom, u, plan, *args)
    for factor in (1.0, 0.375, 3.7):
        ur = u.clone().requires_grad_(True)
        loss = pp.point_loss(geom, ur, plan, *args)
        assert loss.dtype == torch.float32 and float(loss) == float(loss0.float())
        (loss * factor).backward()
        _, gf = pp.point_loss_and_grad(geom, u, plan, *args, gscale=factor)
        assert torch.equal(ur.grad, gf) and torch.equal(ur.grad, torch.tensor(factor, device=dev()) * g0)
    # eval_at_points: random cotangents through the adjoint against the restatement
    g = torch.Generator().manual_seed(5)
    gv, gg = torch.randn((2, 257), generator=g).to(dev()), torch.randn((2, 257, nsd), generator=g).to(dev())
    ur = u.clone().requires_grad_(True)
    vals, grads = pp.eval_at_points(geom, ur, plan, "physical")
    torch.autograd.backward((vals, grads), (gv, gg))
    b, e, xi = plan_arrays(plan)
    ds = ds32(plan, "physical")
    c0 = plan.sort(gv).cpu().numpy().astype(np.float64)
    c = plan.sort(gg, vector=True).cpu().numpy().astype(np.float64).T
    rgrad, agrad, cnt = pr.adjoint((2, *geom.node_shape), b, e, xi, c0, c, ds)
    k = KA[nsd] + (1 + nsd) * cnt + 2
    check("adjoint", f"{nsd}d eval_at_points", np.abs(ur.grad.cpu().numpy().astype(np.float64)[:, 0] - rgrad), k * U / (1.0 - k * U) * agrad)
    # ... and in the caller's order
    rv, rg, av, ag = pr.interpolate(u.cpu().numpy().astype(np.float64)[:, 0], b, e, xi, ds)
    inv = plan.inv.cpu().numpy()
    check("values", f"{nsd}d eval_at_points", np.abs(vals.detach().cpu().numpy().reshape(-1) - rv[inv]), gam(KV[nsd]) * av[inv])
    check("derivatives", f"{nsd}d eval_at_points", np.abs(grads.detach().cpu().numpy().reshape(-1, nsd) - rg[inv]), gam(KD[nsd]) * ag[inv])


@pytest.mark.parametrize("nsd", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dscale", [None, "physical"])
@pytest.mark.parametrize("axes", [None, "transposed"])
def test_points_fused_equals_composed(nsd, kind, dscale, axes):
    from diffnet_amd import points as pp
    geom, u, pts, normals, target = problem(nsd, 65)
    if axes == "transposed":                                      # the same cloud, its columns given in tensor-axis order
        pts, normals = pts.flip(-1).contiguous(), normals.flip(-1).contiguous()
    plan = pp.PointPlan(geom, pts, axes=axes)
    w_val, w_nrm = 0.7, 1.3
    case = f"{nsd}d {kind} {dscale} {axes}"
    fv, fg = pp.eval_at_points(geom, u, plan, dscale)
    cv, cg = pp.eval_at_points_composed(geom, u, plan, dscale)
    b, e, xi = plan_arrays(plan)
    ds = ds32(plan, dscale)
    rv, rg, av, ag = pr.interpolate(u.cpu().numpy().astype(np.float64)[:, 0], b, e, xi, ds)
    ev, eg = (gam(KV[nsd]) + gam(KV_C[nsd])) * av, (gam(KD[nsd]) + gam(KD_C[nsd])) * ag
    inv = plan.inv.cpu().numpy()
    back = [plan.cols.index(c) for c in range(nsd)]               # caller's column c is mesh axis back[c]
    check("fused vs composed", case + " values", np.abs((fv - cv).cpu().numpy().astype(np.float64).reshape(-1)), ev[inv])
    check("fused vs composed", case + " derivatives", np.abs((fg - cg).cpu().numpy().astype(np.float64).reshape(-1, nsd)), eg[inv][:, back])
    # the loss and its gradient: the bounds of u_p and g_d propagated through the penalty and the adjoint
    uf, uc = u.clone().requires_grad_(True), u.clone().requires_grad_(True)
    lf = pp.point_loss(geom, uf, plan, target, normals, kind, w_val, w_nrm, dscale)
    lc = pp.point_terms_composed(geom, uc, plan, target, normals, kind, w_val, w_nrm, dscale)
    lf.backward()
    lc.backward()
    t64 = plan.sort(target).cpu().numpy().astype(np.float64)
    n64 = plan.sort(normals, vector=True).cpu().numpy().astype(np.float64).T
    res = residual_bounds(rv, rg, t64, n64, kind, ev, eg, routes=2)
    lv, ln, c0, c = pr.penalty(rv, rg, t64, n64, kind, w_val, w_nrm)
    bound = loss_bound(res[0][0], res[0][1], w_val, plan.T) + (loss_bound(res[1][0], res[1][1], w_nrm, plan.T * nsd) if kind != "none" else 0.0)
    bound += (gam(plan.T * (1 + nsd) + 4) + 2 * U) * (lv + ln)     # the composed route sums its squares in float32; both losses are rounded to float32
    check("fused vs composed", case + " loss", [abs(float(lf) - float(lc))], [bound])
    e0, ec = cot_bounds(res, c0, c, n64, kind, w_val, w_nrm, routes=2)
    shape = (plan.B, *geom.node_shape)
    _, spread, cnt = pr.adjoint(shape, b, e, xi, e0, ec, ds)       # the cotangents' error bounds, spread like cotangents
    _, agrad, _ = pr.adjoint(shape, b, e, xi, c0, c, ds)
    k = 2 * (KA[nsd] + (1 + nsd) * cnt + 2) + 1 + nsd              # both routes' chains
    check("fused vs composed", case + " gradient", np.abs((uf.grad - uc.grad).cpu().numpy().astype(np.float64)[:, 0]),
          spread + k * U / (1.0 - k * U) * agrad)
