"""The winding-number VJP (csrc/winding_vjp.hip: dn_winding_field_vjp, ops.winding_field_vjp, the autograd wrapper of
diffnet_amd/winding.py) against float64 CPU autograd of winding_ref.winding_general on the same float32 inputs, with a seeded
cotangent g = 2 rnd - 1, for the five parameter sets in use, at every seam of the launch: point counts around the workgroup's 256,
query counts around the LDS chunk of 256, one and several slices of the query range, more slices than chunks.

The comparison is a derived bound, not a chosen tolerance (as test_gpu_winding_field.py):
    |got - ref| <= n * 2^-24 * A,
A the float64 sum over the queries of the absolute values of the terms of that output (winding_vjp_ref.vjp_reference):
    area       |scale|       sum_q |g| sum_j |d_j n_j| inv
    normals_i  |scale| a_p   sum_q |g| |d_i| inv
    points_i   |scale| a_p   sum_q |g| (|n_i| inv + sum_j |d_j n_j| |dinv_i|)
n counts the roundings of the kernel's own loop body on the longest path to one output, in units of 2^-24 (winding_vjp_ref.n_roundings;
the table of test_gpu_winding_field.py for d, the sums and the transcendentals):
  d_i = x_i - q_i                                   1 each, relative to |d_i|
  L1:  s = |d_0| + |d_1| (+ |d_2|)                  dim
       r = v_rcp_f32(s)                             + 2                                                   E_r   = dim + 2
       inv = r^power                                power E_r + (power - 1)                               E_inv
       x = r * (-power)                             E_r + 1                                               E_x
  L2:  r2 = d_0 d_0, fma, fma                       2 + dim
       rs = v_rsq_f32(r2)                           (2 + dim) / 2 + 2                                     E_rs
       inv = rs^power                               power E_rs + (power - 1)                              E_inv
       x = (rs rs) * (-power)                       2 E_rs + 1 + 1                                        E_x
  gi = g * inv                                      E_inv + 1                                             E_gi
  N_i = fma(d_i, gi, N_i)                           the term carries d_i (1) and gi; one rounding per pair of the chunk: 256
  G   = G + gi                                      the term carries gi; 256 for the chain
  num = d_0 n_0, fma, fma                           each product its difference (1), at most dim roundings of the chain: 1 + dim,
                                                    relative to sum_j |d_j n_j|
  cf = (num * gi) * x                               (1 + dim) + E_gi + 1 + E_x + 1
  C_i = fma(d_i, cf, C_i)  /  fma(sgn(d_i), cf, C_i)   L2: the term carries d_i (1) more; L1: sgn is exactly -1, 0 or 1; 256 for the chain
  chunk sums, slices, n . N, n_i G + C_i            float64: below the + 1
  out = float32(scale [a_p] sum)                    scale rounded to float32 (1), the one rounding of the result (1)          = 2
  + 1 for the terms of second order and the float64 operations
=> normals and area (n . N inherits the bound of each N_i, weighted by |n_i|: exactly A_area):
       n = 256 + (1 + E_gi) + 3
   points (n_i G is bounded by the smaller 256 + E_gi + 3 on its own part of A):
       n = 256 + [(1 + dim) + E_gi + 1 + E_x + 1 (+ 1 for L2)] + 3
   3-D L2 cubed: E_rs = 4.5, E_inv = 15.5, E_gi = 16.5, E_x = 11: normals 276.5, points 293.5.
Every point is at least 1e-4 (L1) from every query (asserted on the CPU in test_winding_vjp_host.py).

Largest |got - ref| / (n 2^-24 A) per family on the MI355X, over the three outputs (every test prints its own; run with -s):
    seams    2d_l1_p3 0.050    2d_l1_p2_area 0.051    3d_l1_p3_area 0.030    2d_l2_p2 0.056    3d_l2_p3 0.033
    automatic slices 0.030    L1 sign at zero 0.027    autograd wiring 0.036
(the 256 of the bound is the worst case of a chain of 256 roundings of one sign; the observed errors are those of a random walk)
"""
import math

import pytest
import torch

from test_gpu_parity import dev
import winding_ref as wr
import winding_vjp_ref as vr

RATIOS = {}             # largest ratio to the bound per family in this run
OUTS = ("points", "normals", "area")


def check(family, case, got, ref, A, n):
    r = wr.bound_ratio(got, ref, A, n)
    RATIOS[family] = max(RATIOS.get(family, 0.0), r)
    print(f"winding-vjp-ratio {family} {case}: {r:.3g} (family max so far {RATIOS[family]:.3g})")
    assert r <= 1.0, f"{family} {case}: |got - ref| is {r:.3g} x the bound n 2^-24 A"
    return r


def check_all(family, case, v, got):
    for name, t in zip(OUTS, got):
        if v["ref_" + name] is None:
            assert t is None
            continue
        assert t.dtype == torch.float32 and t.shape == v["ref_" + name].shape
        check(family, f"{case} {name}", t, v["ref_" + name], v["A_" + name], v["n_" + name])


def run(v, slices, want=None):
    from diffnet_amd.ops import winding_field_vjp
    d = dev()
    area = None if v["area"] is None else v["area"].to(d)
    want = want or (OUTS if area is not None else OUTS[:2])
    return winding_field_vjp(v["points"].to(d), v["normals"].to(d), area, v["queries"].to(d), v["g"].to(d), metric=v["metric"],
                             power=v["power"], scale=v["scale"], want=want, slices=slices)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(wr.PARAMS))
def test_vjp_at_workgroup_chunk_and_slice_seams(name):
    for B, npts, nq, slices in vr.SEAMS:
        v = vr.vjp_problem(name, B, npts, nq)
        got = run(v, slices)
        check_all(name, f"B={B} npts={npts} nq={nq} slices={slices}", v, got)
        if v["area"] is None:
            with pytest.raises(ValueError):
                run(v, slices, want=OUTS)


@pytest.mark.gpu
def test_automatic_slices_and_host_queries():
    """slices = 0 gives the bits of the explicit value dn_winding_field_vjp_slices reports; a query tensor left on the host too"""
    from diffnet_amd import _lib
    from diffnet_amd.ops import winding_field_vjp
    B, npts, nq = 2, 257, 3 * 256 + 5
    v = vr.vjp_problem("3d_l1_p3_area", B, npts, nq)
    s = _lib.lib().dn_winding_field_vjp_slices(B, npts, nq)
    assert s == 4                                      # 2^22 / 514 point threads = 8161, cut to the 4 chunks
    auto, explicit = run(v, 0), run(v, s)
    check_all("auto", "3d_l1_p3_area", v, auto)
    d = dev()
    host = winding_field_vjp(v["points"].to(d), v["normals"].to(d), v["area"].to(d), v["queries"], v["g"].to(d), metric="l1", power=3,
                             scale=v["scale"])
    for a, b, c in zip(auto, explicit, host):
        assert torch.equal(a, b) and torch.equal(a, c)
    # a request for more slices than chunks is the request for the chunks
    for a, b in zip(run(v, 9), explicit):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("slices", [1, 3])
def test_two_calls_and_every_subset_give_identical_bits(slices):
    for name in ("3d_l1_p3_area", "2d_l2_p2"):
        v = vr.vjp_problem(name, 2, 257, 3 * 256 + 5)
        a, b = run(v, slices), run(v, slices)
        assert all(torch.equal(x, y) and bool(torch.isfinite(x).all()) for x, y in zip(a, b))
        gp, gn, ga = run(v, slices, want=("normals",))
        assert gp is None and ga is None and torch.equal(gn, a[1])
        gp, gn, ga = run(v, slices, want=("points", "area"))
        assert gn is None and torch.equal(gp, a[0]) and torch.equal(ga, a[2])
        # grad_area comes back in the shape the area was given in
        from diffnet_amd.ops import winding_field_vjp
        d = dev()
        _, _, ga3 = winding_field_vjp(v["points"].to(d), v["normals"].to(d), v["area"].to(d)[..., None].contiguous(), v["queries"].to(d), v["g"].to(d),
                                      metric=v["metric"], power=v["power"], scale=v["scale"], want=("area",), slices=slices)
        assert tuple(ga3.shape) == (2, 257, 1) and torch.equal(ga3[..., 0], a[2])


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_l1_sign_at_zero(dim):
    """query 0 shares coordinate 1 exactly with point k, the one whose normal has the largest x component (L1 distance 0.07): d|d_1| = sgn(0) = 0 as in torch, not copysign's +-1"""
    from diffnet_amd.ops import winding_field_vjp
    name = "2d_l1_p2_area" if dim == 2 else "3d_l1_p3_area"
    p = wr.problem(name, 1, 37, 5)
    q = p["queries"].clone()
    k = int(p["normals"][0, :, 0].abs().argmax())
    q[:, 0] = p["points"][0, k]
    q[0, 0] += 0.07
    assert float(q[1, 0]) == float(p["points"][0, k, 1]) and float((p["points"][0, k] - q[:, 0]).abs().sum()) >= 0.05
    assert float((p["points"][0].double()[None] - q.double().T[:, None]).abs().sum(-1).min()) >= wr.MIN_L1
    g = (2.0 * wr.rnd((1, 5), "g-sign", dim) - 1.0).contiguous()
    g[0, 0] = 1.0                                       # the pair in question weighs in fully
    grads, As = vr.vjp_reference(p["points"].double(), p["normals"].double(), p["area"].double(), q.double(), g.double(), "l1", p["power"], p["scale"])
    # a copysign in the kernel would be off by power |num| s^-(power + 1) a_p, far outside the bound
    dd = (p["points"][0, k] - q[:, 0]).double()
    jump = p["power"] * abs(float((dd * p["normals"][0, k].double()).sum())) * float(dd.abs().sum()) ** -(p["power"] + 1) * float(p["area"][0, k]) * abs(p["scale"])
    nn, npnt = vr.n_roundings(dim, "l1", p["power"])
    assert jump > 100 * npnt * wr.U * float(As[0][0, k, 1])
    d = dev()
    for slices in (1, 2):
        got = winding_field_vjp(p["points"].to(d), p["normals"].to(d), p["area"].to(d), q.to(d), g.to(d), metric="l1", power=p["power"],
                                scale=p["scale"], slices=slices)
        for t, ref, A, n, out in zip(got, grads, As, (npnt, nn, nn), OUTS):
            check("l1 sign", f"{dim}-D slices={slices} {out}", t, ref, A, n)


def _grad_both(fn_gpu, fn_ref, leaves32, c):
    """gradients of (w c).sum() through the fused wrapper on the GPU and through the float64 composite on the CPU"""
    d = dev()
    on = [t.detach().to(d).requires_grad_(t.requires_grad) for t in leaves32]
    w = fn_gpu(*on)
    got = torch.autograd.grad((w * c.to(d)).sum(), [t for t in on if t.requires_grad])
    on64 = [t.detach().double().requires_grad_(t.requires_grad) for t in leaves32]
    ref = torch.autograd.grad((fn_ref(*on64) * c.double()).sum(), [t for t in on64 if t.requires_grad])
    return w, got, ref, on


@pytest.mark.gpu
def test_winding_number_differentiable_5x6x7():
    """the mesh-ordered wrapper: backward goes through its reshape; forward bits are those of the default call"""
    from diffnet_amd.winding import winding_number
    B, npts = 2, 300
    pts, nrm, area = wr.cloud(B, npts, 3, "vjp567")
    x, y, z = torch.linspace(0.0, 1.0, 5), torch.linspace(0.03, 0.97, 6), torch.linspace(0.05, 0.9, 7)
    zz, yy, xx = torch.meshgrid(z, y, x, indexing="ij")
    q = torch.stack((xx, yy, zz)).contiguous()                                  # (3, 7, 6, 5)
    assert float((pts.double()[:, None] - q.reshape(3, -1).double().T[None, :, None]).abs().sum(-1).min()) >= wr.MIN_L1
    c = (2.0 * wr.rnd((B, 1, 7, 6, 5), "c567") - 1.0)
    scale = 1.0 / (4.0 * math.pi)
    area3 = area[..., None].contiguous()
    leaves = [pts.clone().requires_grad_(True), nrm.clone().requires_grad_(True), area3.clone().requires_grad_(True)]

    def ref_fn(p_, n_, a_):
        return wr.winding_general(p_, n_, a_[..., 0], q.reshape(3, -1).double(), "l2", 3, scale)[0].reshape(B, 1, 7, 6, 5)

    d = dev()
    w, got, ref, on = _grad_both(lambda p_, n_, a_: winding_number(p_, n_, a_, q.to(d), differentiable=True), ref_fn, leaves, c)
    assert tuple(w.shape) == (B, 1, 7, 6, 5) and w.requires_grad
    plain = winding_number(*on, q.to(d))
    assert not plain.requires_grad and plain.grad_fn is None and torch.equal(plain, w.detach())
    _, As = vr.vjp_reference(pts.double(), nrm.double(), area.double(), q.reshape(3, -1).double(), c.reshape(B, -1).double(), "l2", 3, scale)
    nn, npnt = vr.n_roundings(3, "l2", 3)
    assert tuple(got[2].shape) == (B, npts, 1)
    check("autograd", "winding_number points", got[0], ref[0], As[0], npnt)
    check("autograd", "winding_number normals", got[1], ref[1], As[1], nn)
    check("autograd", "winding_number area", got[2], ref[2], As[2][..., None], nn)
    # an input that does not require grad gets None, and only what is needed is computed
    leaves2 = [pts.clone(), nrm.clone().requires_grad_(True), area3.clone()]
    on2 = [t.detach().to(d).requires_grad_(t.requires_grad) for t in leaves2]
    w2 = winding_number(*on2, q.to(d), differentiable=True)
    assert torch.equal(w2.detach(), plain)
    (w2 * c.to(d)).sum().backward()
    assert on2[0].grad is None and on2[2].grad is None and torch.equal(on2[1].grad, got[1])
    # ... and the 2-D form without area
    pts2, nrm2, _ = wr.cloud(B, npts, 2, "vjp56")
    yy2, xx2 = torch.meshgrid(y, x, indexing="ij")
    q2 = torch.stack((xx2, yy2)).contiguous()
    c2 = (2.0 * wr.rnd((B, 1, 6, 5), "c56") - 1.0)
    leaves = [pts2.clone().requires_grad_(True), nrm2.clone().requires_grad_(True)]
    s2 = 1.0 / (2.0 * math.pi)
    w, got, ref, _ = _grad_both(lambda p_, n_: winding_number(p_, n_, None, q2.to(d), differentiable=True),
                                lambda p_, n_: wr.winding_general(p_, n_, None, q2.reshape(2, -1).double(), "l2", 2, s2)[0].reshape(B, 1, 6, 5), leaves, c2)
    _, As = vr.vjp_reference(pts2.double(), nrm2.double(), None, q2.reshape(2, -1).double(), c2.reshape(B, -1).double(), "l2", 2, s2)
    nn, npnt = vr.n_roundings(2, "l2", 2)
    check("autograd", "winding_number 2-D points", got[0], ref[0], As[0], npnt)
    check("autograd", "winding_number 2-D normals", got[1], ref[1], As[1], nn)


@pytest.mark.gpu
def test_compute_winding_torch_differentiable_5_cubed():
    """the drop-in with the reference's swapped grid axes: a backward that forgot the transpose would pair c with the wrong probes"""
    from diffnet_amd.winding import compute_winding_torch
    B, npts, n = 2, 37, 5
    pts, nrm, area = wr.cloud(B, npts, 3, "vjp5")
    x = torch.linspace(0.02, 0.98, n)
    q = torch.stack(torch.meshgrid(x, 0.9 * x, 0.8 * x + 0.1, indexing="ij"))[None].contiguous()       # (1, 3, n, n, n), axes that differ
    qf = q[0].reshape(3, -1)
    assert float((pts.double()[:, None] - qf.double().T[None, :, None]).abs().sum(-1).min()) >= wr.MIN_L1
    c = (2.0 * wr.rnd((1, B, n, n, n), "c5") - 1.0)
    area3 = area[..., None].contiguous()
    leaves = [pts.clone().requires_grad_(True), nrm.clone().requires_grad_(True), area3.clone().requires_grad_(True)]

    def ref_fn(p_, n_, a_):                              # out[0, b, j, i, k] = w[b, (i, j, k)]
        return wr.winding_general(p_, n_, a_[..., 0], qf.double(), "l1", 3, 1.0)[0].reshape(1, B, n, n, n).transpose(2, 3)

    d = dev()
    w, got, ref, on = _grad_both(lambda p_, n_, a_: compute_winding_torch(p_, n_, a_, q.to(d), differentiable=True), ref_fn, leaves, c)
    assert tuple(w.shape) == (1, B, n, n, n)
    plain = compute_winding_torch(*on, q.to(d))
    assert not plain.requires_grad and torch.equal(plain, w.detach())
    g_flat = c.transpose(2, 3).reshape(B, -1)            # the cotangent of the flat field
    _, As = vr.vjp_reference(pts.double(), nrm.double(), area.double(), qf.double(), g_flat.double(), "l1", 3, 1.0)
    nn, npnt = vr.n_roundings(3, "l1", 3)
    check("autograd", "compute_winding_torch points", got[0], ref[0], As[0], npnt)
    check("autograd", "compute_winding_torch normals", got[1], ref[1], As[1], nn)
    check("autograd", "compute_winding_torch area", got[2], ref[2], As[2][..., None], nn)
    # the transpose matters for this cotangent: the untransposed pairing is far outside the bound
    wrong, _ = vr.vjp_reference(pts.double(), nrm.double(), area.double(), qf.double(), c.reshape(B, -1).double(), "l1", 3, 1.0)
    assert wr.bound_ratio(wrong[1].float(), ref[1], As[1], nn) > 100.0


@pytest.mark.gpu
def test_example_winding_fit_fused():
    """examples/winding_fit.py --points 400 --n 9 --steps 60 --mode fused: the loss falls by a factor of at least 100 (the composed
    arithmetic gives about 1 000 in float32 and float64; the factor of 10 is headroom for another summation order over 60 Adam steps)"""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("winding_fit", os.path.join(ROOT, "examples", "winding_fit.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    hist = ex.run(mode="fused", n=9, npts=400, steps=60, verbose=False)
    print(f"winding_fit fused: first {hist[0]:.4e} last {hist[-1]:.4e} ratio {hist[0] / hist[-1]:.1f}")
    assert len(hist) == 60 and all(math.isfinite(v) for v in hist)
    assert hist[0] / hist[-1] >= 100.0
