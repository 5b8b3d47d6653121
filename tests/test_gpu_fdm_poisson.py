"""The fused 2-D finite-difference Poisson residual (ops.fdm_poisson_apply, csrc/fdm_poisson.hip) on the GPU: parity with the three
reference fixtures through the DiffNetFDM methods, float64 comparison at the smallest shapes that can break the march, exactness
properties, autograd.  The float64 restatement lives in tests/test_fdm_poisson_host.py.

The comparison is a derived bound, not a chosen tolerance: entry by entry
    |got - ref64| <= k 2^-24 A,
A the same expression with every product replaced by its absolute value (`restate(..., absolute=True)`), k the number of roundings on
the longest path to one output of the kernel (the gamma_k bound; k 2^-24 << 1, and the constants below leave one spare rounding for
its second-order term).  Where A is 0 the output must be exactly 0.

K_RES = 22, the residual.  A horizontal dot product k[m][0] l + k[m][1] c + k[m][2] r is three fmaf, and the three kernel rows of a
stencil are chained into one rolling sum: nine fmaf, nine roundings, for each of kx * u~, ky * u~, kx * nu, ky * nu; kl = kxx + kyy is
rounded once on the host, so kl * u~ has ten.  r = fmaf(nu, lap, fmaf(uy, nuy, fmaf(ux, nux, fs f))): the product ux nux carries
9 + 9 roundings and passes three fmaf: 21; uy nuy 9 + 9 + 2 = 20; nu lap 10 + 1 = 11; fs f 1 + 3 = 4.  Longest: 21, plus the spare.

K_GRAD = 64, the gradient.  a = r (kx * nu) is one product of a value with 21 roundings and one with 9: 31; b likewise, c = r nu 22.
The three adjoint stencils of the three products are chained into one rolling sum over the three rows that reach a node: 27 fmaf, so a
term passes at most 27 more: 58.  The scale 2 out_scale s_b is out_scale rounded to fp32, doubled exactly and multiplied by in_scale[b]:
2 roundings; its product with the sum and the fmaf that adds the Neumann term: 2 more: 62; in the two-launch L2 loss in_scale itself
is a float64 quotient rounded to fp32: 63, plus the spare.  The Neumann term has 2 (the row differences and, for ny = 3, their sum),
3 for 2 out_scale nbc_scale (two conversions, one product) and the fmaf: 6.

Sums.  The kernel squares r in fp64, where the product of two fp32 values is exact, and adds in fp64 -- per thread, then the fixed-order
reduction -- so against the fp64 sum of its OWN fp32 res the only error is that of n additions: n 2^-53 A with A the sum itself (all
terms are positive).  That is tighter than the analogous fp32 bound, which the kernel would also meet.  The two Neumann sums are formed
from the fp32 values of u~ in fp64 (the difference, its square, the additions): (nx + 3) 2^-53 A.

Largest |got - ref| / bound on the MI355X (every test prints its own; run with -s): res 0.095, grad 0.029, sum r^2 0.24, the Neumann
sums 0.19; through the class on the fixtures and the 21^2 batch: gradient 0.0001-0.009, the composed twin's the same size.  The ratios of
res and grad are small because A is far larger than the result for the class's kernels (entries of the order (n - 1)^2 that cancel);
a wrong neighbour or a missed seam row is an error of the order of A: 10^5 bounds or more (profiles/fdm_poisson.txt).
"""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_fdm_poisson_host import FIXTURES, K_GRAD, K_RES, U24, load_fixture, method_args, restate, script_loss, substitute

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53
R = 4                                        # the forced strip height of the seam cases ("PLAN_FSDT" "64,4")


def dev():
    return torch.device("cuda")


def owners():
    """owner columns per wave: the kernel's documented constant"""
    src = open(os.path.join(ROOT, "diffnet_amd", "csrc", "fdm_poisson.hip")).read()
    return int(re.search(r"constexpr int FDM_OWNERS = (\d+);", src).group(1))


@pytest.fixture
def plan():
    from diffnet_amd import _lib
    assert _lib.config_get("PLAN_FSDT") == ""

    def set_(value):
        _lib.config_set("PLAN_FSDT", value)

    yield set_
    _lib.config_set("PLAN_FSDT", "")


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
FIELD_VARIANTS = ("none", "const", "shared", "batched")
MASK_VARIANTS = ("none", "one_f32_shared", "second_u8_batched_field", "two_f32_batched_bool_shared_field", "two_frame_u8_f32")
KERNEL_VARIANTS = ("fdm", "sobel", "random")


def edge_mask(rng, shape, p):
    """a random mask that also touches the first and last two rows and columns"""
    m = rng.random(shape) < p
    ny, nx = shape[-2:]
    for y, x in ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1), (1, 1), (ny - 2, nx - 2), (1, nx - 2), (ny - 2, 1), (0, nx // 2), (ny - 1, nx // 2)):
        m[..., y, x] = True
    m[..., ny // 2, nx // 2] = False
    return m


def make_case(B, ny, nx, nuv, fv, mv, kv, seed):
    from diffnet_amd import ops
    from diffnet_amd.fdm import get_deriv_kernels
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    c = dict(B=B, ny=ny, nx=nx, u=f32(rng.standard_normal((B, 1, ny, nx))))
    field = lambda v, gen: {"none": None, "const": float(np.float32(gen(()))), "shared": f32(gen((1, 1, ny, nx))), "batched": f32(gen((B, 1, ny, nx)))}[v]
    c["nu"] = field(nuv, lambda s: 0.5 + rng.random(s))
    c["f"] = field(fv, lambda s: rng.standard_normal(s))
    full, one = (B, 1, ny, nx), (1, 1, ny, nx)
    if mv == "none":
        masks, vals = (None, None), (0.0, 0.0)
    elif mv == "one_f32_shared":
        masks, vals = (f32(edge_mask(rng, one, 0.25)), None), (0.75, 0.0)
    elif mv == "second_u8_batched_field":
        masks, vals = (None, edge_mask(rng, full, 0.25).astype(np.uint8) * 3), (0.0, f32(rng.standard_normal(one)))
    elif mv == "two_f32_batched_bool_shared_field":
        masks, vals = (f32(edge_mask(rng, full, 0.2)) * 0.75, edge_mask(rng, one, 0.2)), (-0.5, f32(rng.standard_normal(full)))
    else:
        frame = np.zeros(one, np.uint8)
        frame[..., :2, :] = frame[..., -2:, :] = frame[..., :, :2] = frame[..., :, -2:] = 1
        frame[..., ::2, ::3] = 0
        masks, vals = (frame, f32(rng.random(full) < 0.15)), (1.0, 0.25)
    c["masks"], c["vals"] = masks, vals
    if kv == "fdm":
        c["kernels"], c["ks"] = None, tuple(np.asarray(k, np.float64).reshape(3, 3) for k in ops.fdm_default_kernels(nx))
    else:
        if kv == "sobel":
            _, kx, ky, _, _, kxx, kyy, _ = get_deriv_kernels(2, "sobel", 3, nx)
            ks = tuple(f32(k) for k in (kx, ky, kxx, kyy))
        else:
            ks = tuple(f32(rng.standard_normal((3, 3))) for _ in range(4))
        c["kernels"], c["ks"] = ks, ks
    c["fs"], c["out_scale"], c["nbc_scale"] = 0.625, 0.37, 1.3      # fs exact in fp32; the roundings of the two scales are counted in K_GRAD
    c["in_scale"] = f32(0.5 + rng.random(B))
    return c


def t(a):
    return a if a is None or isinstance(a, float) else torch.as_tensor(a).to(dev())


def apply(c, want=(True, True, True), in_scale=True, **over):
    from diffnet_amd import ops
    kw = dict(nu=t(c["nu"]), f=t(c["f"]), bc=tuple(t(m) for m in c["masks"]), bc_values=tuple(t(v) for v in c["vals"]),
              kernels=None if c["kernels"] is None else tuple(torch.as_tensor(k) for k in c["kernels"]), fs=c["fs"], out_scale=c["out_scale"],
              nbc_scale=c["nbc_scale"], want_res=want[0], want_grad=want[1], want_sums=want[2],
              in_scale=in_scale if isinstance(in_scale, torch.Tensor) else (t(c["in_scale"]) if in_scale else None))
    kw.update(over)
    return ops.fdm_poisson_apply(t(c["u"]), **kw)


def reference(c, absolute=False, in_scale=True):
    return restate(c["u"], 1.0 if c["nu"] is None else c["nu"], 0.0 if c["f"] is None else c["f"], c["fs"], c["ks"], c["masks"], c["vals"],
                   c["out_scale"], c["nbc_scale"], c["in_scale"] if in_scale else None, absolute=absolute)


def ratio(got, ref, bound):
    """largest |got - ref| / bound; entries with a zero bound must be exact"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(err).all()
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def check(c, want=(True, True, True), tag=""):
    grad, sums, res = apply(c, want)
    assert (grad is None, sums is None, res is None) == (not want[1], not want[2], not want[0])
    r64, s64, g64 = reference(c)
    ra, sa, ga = reference(c, absolute=True)
    out = {}
    if want[0]:
        assert res.shape == (c["B"], 1, c["ny"] - 2, c["nx"] - 2) and res.dtype == torch.float32
        out["res"] = ratio(res.cpu().numpy(), r64, K_RES * U24 * ra)
    if want[1]:
        assert grad.shape == c["u"].shape and grad.dtype == torch.float32
        out["grad"] = ratio(grad.cpu().numpy(), g64, K_GRAD * U24 * ga)
        _, fixed = substitute(c["u"], c["masks"], c["vals"])
        assert (grad.cpu().numpy()[fixed] == 0.0).all()                  # exactly zero on the Dirichlet nodes
    if want[2]:
        assert sums.shape == (c["B"], 3) and sums.dtype == torch.float64
        s = sums.cpu().numpy()
        nin = (c["ny"] - 2) * (c["nx"] - 2)
        if want[0]:                          # against the fp64 sum of the kernel's own fp32 res
            own = (res.cpu().numpy().astype(np.float64) ** 2).sum((1, 2, 3))
            out["sum_r2"] = ratio(s[:, 0], own, (nin + 1) * U53 * own)
        else:                                # ... or, without it, by the bound of the residual: d(r^2) <= (2 K_RES + 1) u A_r^2
            out["sum_r2"] = ratio(s[:, 0], s64[:, 0], (2 * K_RES + 1) * U24 * sa[:, 0])
        out["sum_nbc"] = ratio(s[:, 1:], s64[:, 1:], (c["nx"] + 3) * U53 * s64[:, 1:])
    for k, v in out.items():
        assert v <= 1.0, (tag, k, v)
    return out


def report(name, ratios):
    keys = sorted({k for r in ratios for k in r})
    print(f"\n{name}: largest |got - ref| / bound: " + "  ".join(f"{k} {max(r.get(k, 0.0) for r in ratios):.3g}" for k in keys))


# ---------------------------------------------------------------------------------------------
# parity with the reference fixtures, through the class
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(FIXTURES))
def test_fixture_parity_through_the_class_methods(case):
    from diffnet_amd.fdm import DiffNetFDM
    z, u, nu, f, ks, masks, vals = load_fixture(case)
    loss64, lb, grad64, gb = script_loss(case, u, nu, f, ks, masks, vals)
    m = DiffNetFDM(None, domain_size=int(z["n"])).to(dev())
    kw = method_args(case, nu, f, masks, vals, lambda a: torch.tensor(a).to(dev()))
    ud = torch.tensor(u).to(dev())
    loss, grad = m.poisson_residual_loss_and_grad(ud, **kw)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    g = grad.cpu().numpy().astype(np.float64)
    print(f"\n{case}: loss {float(loss):.9g} fixture {float(z['loss_mean']):.9g} float64 {loss64:.12g} bound {lb:.3g}; "
          f"gradient |got - ref64| / bound {float((np.abs(g - grad64) / np.maximum(gb, 1e-300)).max()):.3g}")
    assert abs(float(loss) - loss64) <= lb and abs(float(loss) - float(z["loss_mean"])) <= 2 * lb     # both within the bound of float64
    assert (np.abs(g - grad64) <= gb).all() and (np.abs(g - z["grad"]) <= 2 * gb).all()
    # ... and by autograd
    ur = ud.clone().requires_grad_(True)
    l2 = m.poisson_residual_loss(ur, **kw)
    l2.backward()
    assert torch.equal(l2.detach(), loss) and torch.equal(ur.grad, grad)
    # the composed twin on the device
    uc = ud.clone().requires_grad_(True)
    lc = m.composed_poisson_residual_loss(uc, **kw)
    gc, = torch.autograd.grad(lc, uc)
    assert abs(float(lc.detach()) - float(z["loss_mean"])) <= 2 * lb
    assert (np.abs(gc.cpu().numpy().astype(np.float64) - z["grad"]) <= 2 * gb).all()


# ---------------------------------------------------------------------------------------------
# float64 at the shapes that can break the march
# ---------------------------------------------------------------------------------------------
def seam_shapes():
    n = owners()
    shapes = [(3, 3), (3, 5), (4, 4), (5, 3)]
    shapes += [(5, w) for w in (n - 1, n, n + 1, n + 2, 2 * n - 1, 2 * n, 2 * n + 1, 2 * n + 2)]       # around one and two waves' owner columns
    shapes += [(h, 7) for h in (R - 1, R, R + 1, R + 2, 2 * R + 1)]                                    # around the forced strip height
    shapes += [(2 * R + 1, n + 2), (R + 2, 2 * n + 1)]                                                 # both seams at once
    return shapes


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("shape", seam_shapes(), ids=lambda s: f"{s[0]}x{s[1]}")
def test_float64_at_chunk_and_strip_seams(shape, B, plan):
    plan(f"64,{R}")
    ny, nx = shape
    i = seam_shapes().index(shape) * 2 + (B > 1)
    # every option of every argument appears along the list (cycles of coprime lengths 4, 3, 5, 3)
    c = make_case(B, ny, nx, FIELD_VARIANTS[i % 4], FIELD_VARIANTS[(i // 4 + i) % 4], MASK_VARIANTS[i % 5], KERNEL_VARIANTS[i % 3], 1000 + i)
    report(f"{ny}x{nx} B={B}", [check(c, tag=(shape, B))])


@pytest.mark.parametrize("mv", MASK_VARIANTS)
def test_float64_over_fields_masks_and_kernels(mv, plan):
    plan(f"64,{R}")
    n = owners()
    ratios = []
    for a, nuv in enumerate(FIELD_VARIANTS):
        for b, fv in enumerate(FIELD_VARIANTS):
            for k, kv in enumerate(KERNEL_VARIANTS):
                c = make_case(3, R + 2, n + 3, nuv, fv, mv, kv, 2000 + 100 * a + 10 * b + k)
                ratios.append(check(c, tag=(mv, nuv, fv, kv)))
    report(mv, ratios)


def test_float64_under_the_default_plan_with_several_strips_and_workgroups():
    # 70 rows: the library's own plan cuts them into strips of at most 18; three chunks, batch 3: more than one workgroup per sample
    ratios = [check(make_case(3, 70, 2 * owners() + 5, "batched", "shared", MASK_VARIANTS[3], kv, 3000 + k)) for k, kv in enumerate(KERNEL_VARIANTS)]
    report("default plan", ratios)


# ---------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------
def test_bitwise_independent_of_the_batch_and_of_the_plan(plan):
    n = owners()
    c = make_case(3, 2 * R + 3, n + 7, "batched", "batched", MASK_VARIANTS[3], "random", 4000)
    plan(f"64,{R}")
    grad, sums, res = apply(c)
    sums2 = apply(c)[1]
    assert torch.equal(sums, sums2)                                      # a fixed-order reduction: reproducible
    for b in range(3):                       # a sample alone
        one = dict(c, B=1, u=c["u"][b:b + 1], nu=c["nu"][b:b + 1], f=c["f"][b:b + 1], in_scale=c["in_scale"][b:b + 1],
                   masks=(c["masks"][0][b:b + 1], c["masks"][1]), vals=(c["vals"][0], c["vals"][1][b:b + 1]))
        g1, s1, r1 = apply(one)
        assert torch.equal(g1[0], grad[b]) and torch.equal(r1[0], res[b])
        assert torch.equal(s1[0], sums[b])                               # the per-sample reduction adds the sample's own partials only
    for value in ("128,3", "256,1", f"64,{2 * R + 3}", ""):              # other strips, other workgroups, one strip, the library's plan
        plan(value)
        g2, s2, r2 = apply(c)
        assert torch.equal(g2, grad) and torch.equal(r2, res), value
        # another plan adds the same positive fp64 terms in another order: at most one rounding per node either way
        np.testing.assert_allclose(s2.cpu().numpy(), sums.cpu().numpy(), rtol=2 * c["ny"] * c["nx"] * U53, atol=0)


def test_in_scale_and_nbc_scale_act_as_specified():
    c = make_case(3, 9, 23, "shared", "batched", MASK_VARIANTS[1], "sobel", 5000)
    base = apply(c, (False, True, False), in_scale=False, nbc_scale=0.0)[0]
    ones = apply(c, (False, True, False), in_scale=torch.ones(3, device=dev()), nbc_scale=0.0)[0]
    assert torch.equal(base, ones)
    # powers of two scale the residual part exactly, sample by sample
    pw = torch.tensor([2.0, 0.5, -4.0], device=dev())
    got = apply(c, (False, True, False), in_scale=pw, nbc_scale=0.0)[0]
    assert torch.equal(got, base * pw.reshape(3, 1, 1, 1))
    # the Neumann part alone: in_scale = 0 leaves out_scale nbc_scale d(down + up)/du, non-zero on the two rows at either end only
    nb = apply(c, (False, True, False), in_scale=torch.zeros(3, device=dev()))[0].cpu().numpy()
    ut, fixed = substitute(c["u"], c["masks"], c["vals"])
    assert (nb[:, :, 2:-2] == 0).all()
    d0, d1 = ut[:, :, 0] - ut[:, :, 1], ut[:, :, -1] - ut[:, :, -2]
    want = np.zeros_like(ut)
    want[:, :, 0], want[:, :, 1], want[:, :, -1], want[:, :, -2] = 2 * d0, -2 * d0, 2 * d1, -2 * d1
    want = np.where(fixed, 0.0, c["out_scale"] * c["nbc_scale"] * want)
    mag = np.zeros_like(ut)
    mag[:, :, 0] = mag[:, :, 1] = np.abs(ut[:, :, 0]) + np.abs(ut[:, :, 1])
    mag[:, :, -1] = mag[:, :, -2] = np.abs(ut[:, :, -1]) + np.abs(ut[:, :, -2])
    assert ratio(nb, want, 6 * U24 * 2 * abs(c["out_scale"] * c["nbc_scale"]) * np.where(fixed, 0.0, mag)) <= 1.0
    # ny = 3: the middle row takes both Neumann terms
    report("ny = 3", [check(make_case(2, 3, 11, "const", "none", MASK_VARIANTS[0], "fdm", 5001))])


@pytest.mark.parametrize("want", [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True),
                                  (False, True, True), (True, True, True)], ids=lambda w: "".join(n for n, on in zip(("res", "grad", "sums"), w) if on))
def test_every_output_combination_returns_what_was_asked_for(want, plan):
    plan(f"64,{R}")
    c = make_case(2, R + 3, owners() + 2, "shared", "batched", MASK_VARIANTS[2], "random", 6000)
    report(str(want), [check(c, want)])
    if want[1]:                              # the gradient does not depend on which other outputs ride along
        assert torch.equal(apply(c, want)[0], apply(c)[0])


# ---------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(FIXTURES))
def test_autograd_matches_the_explicit_gradient_and_the_composed_twin(case):
    from diffnet_amd.fdm import DiffNetFDM
    n, B = 21, 3
    c = make_case(B, n, n, "batched", "batched", "two_f32_batched_bool_shared_field" if case != "mms" else "one_f32_shared", "fdm", 7000)
    masks, vals = c["masks"], c["vals"]
    m = DiffNetFDM(None, domain_size=n).to(dev())
    kw = method_args(case, c["nu"], c["f"], masks, vals, t)
    kw["bc_values"] = tuple(t(v) for v in vals)
    ud = t(c["u"])
    loss, grad = m.poisson_residual_loss_and_grad(ud, **kw)
    ur = ud.clone().requires_grad_(True)
    la = m.poisson_residual_loss(ur, **kw)
    (3.0 * la).backward()
    assert torch.equal(la.detach(), loss) and torch.equal(ur.grad, grad * 3.0)
    assert m.poisson_residual_loss(ud, **kw).requires_grad is False
    uc = ud.clone().requires_grad_(True)
    lc = m.composed_poisson_residual_loss(uc, **kw)
    gc, = torch.autograd.grad(lc, uc)
    loss64, lb, grad64, gb = script_loss(case, c["u"], c["nu"], c["f"], c["ks"], masks, vals)
    g, gcn = grad.cpu().numpy().astype(np.float64), gc.cpu().numpy().astype(np.float64)
    print(f"\n{case}: |fused - float64| / bound {float((np.abs(g - grad64) / np.maximum(gb, 1e-300)).max()):.3g}, "
          f"|composed - float64| / bound {float((np.abs(gcn - grad64) / np.maximum(gb, 1e-300)).max()):.3g}")
    assert abs(float(loss) - loss64) <= lb and (np.abs(g - grad64) <= gb).all()
    assert abs(float(loss) - float(lc.detach())) <= 2 * lb and (np.abs(g - gcn) <= 2 * gb).all()      # each within the bound of float64
