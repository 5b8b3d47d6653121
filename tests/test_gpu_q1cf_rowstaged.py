"""The closed-form 2-D Q1 kernel with the row-staged stiffness element and the one-condition mask forms (poisson2d_q1_cf.hip), on the
launches where it takes another path: seams and a row count off the strip height (16 x 9, 20 x 11 nodes under PLAN2D 64,4,3), two
elements per thread (18 x 9), rows of 4 k + 1 nodes (321 x 9), chained strips (512 x 17 under PLAN2D 128,4,2,4); B = 1 and 3; no
condition, box faces alone, one packed, packed + box faces, one uint8 image, two uint8 images, one fp32 mask with a value field (the form that keeps the
element on raw nodal values); each with and without nu and f.  Every launch
  - against the float64 oracle at the suite's tolerances (scalars rtol 1e-5, gradients rtol 1e-4 + 1e-4 max|ref|, residual fields
    rtol 1e-5 + 1e-6 max|ref|),
  - against the per-point kernel (Q1_RULE_KERNEL; it takes mask images only, so packed masks and box faces go to it as uint8 images of
    the same nodes) at 2e-6,
  - twice, for bitwise equality."""
import numpy as np
import pytest
import torch

from test_gpu_parity import dev, module
from test_gpu_switch_invariance import _conds, _kw2, _np, _oracle, _sentinel, seeded

pytestmark = pytest.mark.gpu

SHAPES = {"16x9": ((16, 9), "64,4,3"), "20x11": ((20, 11), "64,4,3"), "18x9": ((18, 9), None), "321x9": ((321, 9), None),
          "512x17": ((512, 17), "128,4,2,4")}
MASKS = {"none": [], "box": [("box", "box")], "packed": [("packed", "box")], "packed_box": [("packed", "obj"), ("box", "box")], "u8": [("u8", "box")],
         "u8_u8": [("u8", "obj"), ("u8", "box")], "value": [("value", "obj")]}
AS_IMAGES = {"packed": "u8", "box": "u8"}


@pytest.fixture
def switch():
    from diffnet_amd import _lib
    held = []

    def set_(key, value):
        held.append(key)
        _lib.config_set(key, value)

    yield set_
    for key in held:
        _lib.config_set(key, "")


def _launches(m, B, ud, nud, fd, dg, c, jac):
    """energy form, residual form and the form with alpha = 0, each launched twice: {name: (kind, tensor)} of the second launch, after the bitwise comparison"""
    from diffnet_amd import ops
    scale = 1.0 / (B * m.geom.nelem_total)
    res = {}
    for name, kw in (("energy", dict(alpha=2.0 * c, beta=1.0, c=c, out_scale=scale, loss_scale=scale)), ("residual", dict(alpha=1.0, beta=1.0, c=0.0, out_scale=1.0)),
                     ("c0", dict(alpha=0.0, beta=1.0, c=1.0, out_scale=1.0))):       # alpha = 0: the stiffness sum without its cotangents
        p = ops.PoissonPlan(m.geom, ud, nud, fd, None, dg, wscale=jac, want_out=True, want_sums=True, strict=False, **kw)
        _sentinel(*p.result)
        first = [t.clone() for t in (p.launch()[0], p.result[1])]
        torch.cuda.synchronize()
        _sentinel(*p.result)
        p.launch()
        torch.cuda.synchronize()
        out, sums = p.result[0], p.result[1]
        assert torch.equal(first[0], out) and torch.equal(first[1], sums), f"{name}: two identical launches differ"
        res[name + "_out"] = ("g" if name == "energy" else "f", out.clone())
        res[name + "_e"] = ("s", sums[0].clone())
        res[name + "_sumsq"] = ("s", sums[1].clone())
    return res


@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_rowstaged_kernel(shape, B, mask, switch):
    sizes, plan = SHAPES[shape]
    kw = _kw2(sizes[0], 3, sizes=sizes)
    m = module(kw)
    full = (B, 1, *m.geom.node_shape)
    seed = 1000 + 17 * sorted(SHAPES).index(shape) + 5 * B
    u, nuv, f = seeded(full, seed), seeded(full, seed + 1, 0.5), seeded(full, seed + 2)
    dg, dr, masks = _conds(full, MASKS[mask], seed + 4)
    di, _, _ = _conds(full, [(AS_IMAGES.get(form, form), kind) for form, kind in MASKS[mask]], seed + 4)
    o = _oracle(kw)
    c, jac = 0.5, 0.7
    scale = 1.0 / (B * m.geom.nelem_total)
    for has_nu in (True, False):
        for has_f in (True, False):
            tag = f"{shape} B={B} {mask} nu={has_nu} f={has_f}"
            ud, nud, fd = u.to(dev()), (nuv.to(dev()) if has_nu else None), (f.to(dev()) if has_f else None)
            if plan:
                switch("PLAN2D", plan)
            got = _launches(m, B, ud, nud, fd, dg, c, jac)
            switch("PLAN2D", "")
            switch("Q1_RULE_KERNEL", "1")
            rule = _launches(m, B, ud, nud, fd, di, c, jac)
            switch("Q1_RULE_KERNEL", "")
            # float64 oracle
            a = dict(nu=nuv.double() if has_nu else None, f=f.double() if has_f else None, dirichlet=dr)
            ur = u.double().requires_grad_(True)
            e = o.energy(ur, c=c, jac=jac, **a)
            (ge,) = torch.autograd.grad(e, ur)
            R = o.residual(u.double(), jac=jac, zero_masks=masks, **a)
            e1 = o.energy(u.double(), c=1.0, jac=jac, **a) / scale
            ref = dict(c0_e=_np(e1), energy_out=_np(ge), energy_e=_np(e) / scale, energy_sumsq=float(np.sum(_np(ge) ** 2)) / scale ** 2,
                       residual_out=_np(R), residual_sumsq=float(np.sum(_np(R) ** 2)))
            for k, (kind, t) in got.items():
                x, y = _np(t), _np(rule[k][1])
                assert np.isfinite(x).all(), f"{tag} {k}: non-finite (an output left unwritten)"
                if kind == "s":
                    np.testing.assert_allclose(x, y, rtol=2e-6, err_msg=f"{tag} {k} against the per-point kernel")
                else:
                    np.testing.assert_allclose(x, y, rtol=0, atol=2e-6 * max(1e-30, float(np.abs(y).max())), err_msg=f"{tag} {k} against the per-point kernel")
                if k not in ref:          # (the residual form's energy slot, c = 0: minus the forcing work; the forcing-only field of alpha = 0)
                    continue
                r = np.asarray(ref[k], dtype=np.float64).reshape(x.shape)
                if kind == "s":
                    np.testing.assert_allclose(x, r, rtol=1e-5, err_msg=f"{tag} {k} against the float64 oracle")
                else:
                    rt, at = (1e-4, 1e-4) if kind == "g" else (1e-5, 1e-6)
                    np.testing.assert_allclose(x, r, rtol=rt, atol=at * max(1e-30, float(np.abs(r).max())), err_msg=f"{tag} {k} against the float64 oracle")
