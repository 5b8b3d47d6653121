"""Every tuning switch of dn_config_set against every operator form (include/diffnet_hip.h: "every setting yields the same results to
rounding").  Each pair (setting, case) must either
  (a) match the float64 oracle within the suite's tolerances (test_gpu_parity.py) AND the no-switch run within rounding (2e-6 relative for
      scalars, 2e-6 * max|ref| for fields), or
  (b) raise DiffNetHipError, and be listed in EXPECTED_REFUSALS with its reason.
An unlisted refusal fails, and so does a listed one that no longer happens.  Prepared launches get their output and scalar slots filled with
NaN / -1 before every launch, so an output a launch leaves unwritten fails too.

The cases cross the condition forms (fp32 / uint8 images, PackedMask, BoxFaces, value fields, f_gp, LoadVector) and the chained launches
(PoissonPlan fold / strip_select / async_sums, FSDT defer_norms -> norms_from) with the meshes where kernels go wrong: 4 k + 1 / 4 k + 2 /
4 k wide rows, row counts that are no multiple of a strip height, odd and even 3-D x extents, batches of 1 and 3."""
import fnmatch
import os
import re

import numpy as np
import pytest
import torch

from test_gpu_parity import boundary_mask, dev, module, seeded

pytestmark = pytest.mark.gpu

ON_OFF = ["Q1_RULE_KERNEL", "GPE_GATHER", "GPE_TILED", "Q1_3D_T16", "Q1_3D_E1SUM", "Q1_3D_E1", "FSDT_GENERIC", "CONV2D_V1", "Q1_3D_N2"]
SETTINGS = ([("PLAN2D", v) for v in ("64,2,8", "128,4,7", "128,4,7,2")] + [("PLAN3D", v) for v in ("16,16,1,5", "16,16,2,3", "32,8,1,4")] +
            [("PLAN_FSDT", v) for v in ("64,7", "192,4", "64,4,2")] + [("FSDT_FORM", v) for v in ("elem", "stencil")] +
            [("CONV_WRW_WGS", v) for v in ("256", "4096")] + [(k, "1") for k in ON_OFF])
NOT_CROSSED = {"HANDOVER_SPIN_LIMIT"}          # a fault-injection hook (test_gpu_round4.py: test_chained_strip_handover_timeout_is_loud)

# (key, value or None for any, case glob) -> reason.  Only switch settings: the default setting runs every case.
EXPECTED_REFUSALS = {
    ("Q1_3D_T16", None, "p3d_*load*"): "load vectors are taken by the 3-D two-element kernel only; the switch turns that form off",
    ("Q1_3D_E1", None, "p3d_*load*"): "load vectors are taken by the 3-D two-element kernel only; the switch turns that form off",
    ("Q1_3D_T16", None, "fold3d_*"): "fold_prev exists in the 3-D two-element kernel only; the switch turns that form off",
    ("Q1_3D_E1", None, "fold3d_*"): "fold_prev exists in the 3-D two-element kernel only; the switch turns that form off",
    ("Q1_RULE_KERNEL", None, "fold2d_*"): "fold_prev exists in the 2-D closed-form Q1 kernel only; the switch turns that kernel off",
}


def _refusal_reason(key, value, case):
    for (k, v, pat), why in EXPECTED_REFUSALS.items():
        if k == key and (v is None or v == value) and fnmatch.fnmatch(case, pat):
            return why
    return None


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def _sentinel(*ts):
    for t in ts:
        if isinstance(t, torch.Tensor):
            t.fill_(float("nan") if t.dim() > 1 else -1.0)


def _blob(shape, seed, frac=0.05):
    return (seeded(shape, seed) < frac).float()


def _kw2(n, ngp, deg=1, sizes=None):
    kw = dict(domain_size=n, ngp_1d=ngp, fem_basis_deg=deg)
    if sizes is not None:
        kw.update(domain_sizes=sizes, domain_lengths=tuple(0.02 * (s - 1) for s in sizes), domain_size=sizes[0],
                  domain_length=0.02 * (sizes[0] - 1))
    return kw


def _cond_gpu(form, mask, value):
    """One Dirichlet condition in the named form (mask: float CPU image)."""
    from diffnet_amd import BoxFaces, PackedMask
    if form == "box":
        return (BoxFaces("all"), value)
    d = mask.to(dev())
    if form == "u8":
        d = d.to(torch.uint8)
    elif form == "packed":
        d = PackedMask.pack(d)
    if isinstance(value, torch.Tensor):
        value = value.to(dev())
    return (d, value)


def _conds(shape, spec, seed):
    """spec: list of (form, kind) with kind "box" (all faces, value 0) or "obj" (a blob off the boundary, value 1 or a value field)."""
    box = boundary_mask((1,) + tuple(shape[1:]))
    obj = _blob((1,) + tuple(shape[1:]), seed, 0.05) * (1 - box)
    gpu, ref = [], []
    for form, kind in spec:
        if kind == "box":
            gpu.append(_cond_gpu(form, box, 0.0))
            ref.append((box.double(), 0.0))
        else:
            val = seeded((1,) + tuple(shape[1:]), seed + 7) if form == "value" else 1.0
            gpu.append(_cond_gpu("f32" if form == "value" else form, obj, val))
            ref.append((obj.double(), val.double() if isinstance(val, torch.Tensor) else val))
    return gpu, ref, [m for m, _ in ref]


def _oracle(kw):
    """The oracle (the reference formulation on CPU torch) with its tables in float64."""
    from oracle.fem_oracle import Oracle
    o = Oracle(**kw)
    o.t = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in o.t.items()}
    o.gpw = o.gpw.double()
    return o


# ---------------------------------------------------------------------------------------------
# cases: name -> builder returning (gpu(), ref()) -- gpu() gives {name: (kind, tensor)}, ref() {name: float64 array}
# kind: "s" scalar (rtol 1e-5), "f" field (rtol 1e-5, atol 1e-6 max|ref|), "g" gradient (rtol 1e-4, atol 1e-4 max|ref|), "c" / "w" convolution
# output / weight gradient (max error 2e-5 / 4e-5 of max|ref|)
# ---------------------------------------------------------------------------------------------
CASES = {}


def _case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


def _poisson_case(kw, B, spec, seed, nu=True, force="f", residual=True, c=0.5, jac=0.7):
    def build():
        from diffnet_amd import LoadVector, ops
        m = module(kw)
        shape = (B, 1, *m.geom.node_shape)
        u, nuv, f = seeded(shape, seed), seeded(shape, seed + 1, 0.5), seeded(shape, seed + 2)
        fgp = seeded((1, m.geom.ngp_total, *m.geom.elem_shape), seed + 3) if force == "fgp" else None
        dg, dr, masks = _conds(shape, spec, seed + 4)
        nu_h = nuv if nu else None
        ud, nud, fd = u.to(dev()), (nuv.to(dev()) if nu else None), f.to(dev())
        fgd = None if fgp is None else fgp.to(dev())
        f_arg = None if force == "fgp" else fd
        scale = 1.0 / (B * m.geom.nelem_total)

        def gpu():
            fa = LoadVector.assemble(m.geom, fd) if force == "load" else f_arg
            res = {}
            p = ops.PoissonPlan(m.geom, ud, nud, fa, fgd, dg, alpha=2.0 * c, beta=1.0, c=c, wscale=jac, out_scale=scale, want_out=True,
                                want_sums=True, loss_scale=scale, strict=False)
            _sentinel(*p.result)
            out, sums, loss = p.launch()
            res.update(energy_loss=("s", loss), energy_grad=("g", out), energy_sum=("s", sums[0]))
            # one-shot route (mask images are packed on first use where the compact kernels run)
            g1 = torch.full_like(ud, float("nan"))
            l1, g1 = ops.energy_loss_and_grad(m.geom, ud, nud, fa, fgd, dg, c=c, jac=jac, out=g1)
            res.update(oneshot_loss=("s", l1), oneshot_grad=("g", g1))
            if residual:
                p = ops.PoissonPlan(m.geom, ud, nud, fa, fgd, dg, alpha=1.0, beta=1.0, c=0.0, wscale=jac, out_scale=1.0, want_out=True,
                                    want_sums=True, strict=False)
                _sentinel(*p.result)
                R, sums = p.launch()
                ug = ud.clone().requires_grad_(True)
                rl = ops.residual_loss(m.geom, ug, nud, fa, fgd, dg, jac=jac)
                (gr,) = torch.autograd.grad(rl, ug)
                res.update(residual=("f", R), residual_sumsq=("s", sums[1]), residual_loss=("s", rl), residual_grad=("g", gr))
            return res

        def ref():
            o = _oracle(kw)
            ur = u.double().requires_grad_(True)
            a = dict(nu=None if nu_h is None else nu_h.double(), f=None if force == "fgp" else f.double(),
                     f_gp=None if fgp is None else fgp.double(), dirichlet=dr)
            e = o.energy(ur, c=c, jac=jac, **a)
            (ge,) = torch.autograd.grad(e, ur)
            out = dict(energy_loss=_np(e), energy_grad=_np(ge), energy_sum=_np(e) / scale, oneshot_loss=_np(e), oneshot_grad=_np(ge))
            if residual:
                ur = u.double().requires_grad_(True)
                if kw.get("fem_basis_deg", 1) == 1:
                    R = o.residual(ur, jac=jac, zero_masks=masks, **a)
                else:
                    a.pop("f_gp")
                    R = o.residual_any_degree(ur, jac=jac, zero_masks=masks, **a)
                L = torch.sum(R ** 2)
                (gr,) = torch.autograd.grad(L, ur)
                out.update(residual=_np(R), residual_sumsq=_np(L), residual_loss=_np(L), residual_grad=_np(gr))
            return out

        return gpu, ref
    return build


# 2-D Poisson: Q1 with 2 / 3 / 4 points and Q2; rows of 4 k + 2, 4 k + 1 and 4 k nodes; row counts off any strip height; B = 1 and 3
_case("p2d_q1g2_n66_B1_u8")(_poisson_case(_kw2(66, 2), 1, [("u8", "obj"), ("u8", "box")], 10))
_case("p2d_q1g3_n65_B3_f32")(_poisson_case(_kw2(65, 3), 3, [("f32", "obj"), ("f32", "box")], 20))
_case("p2d_q1g4_n64_B3_packed")(_poisson_case(_kw2(64, 4), 3, [("packed", "obj"), ("packed", "box")], 30, c=1.0))
_case("p2d_q1g3_72x45_B1_box_packed")(_poisson_case(_kw2(72, 3, sizes=(72, 45)), 1, [("packed", "obj"), ("box", "box")], 40))
_case("p2d_q1g2_130x37_B1_box")(_poisson_case(_kw2(130, 2, sizes=(130, 37)), 1, [("box", "box")], 45, nu=False))
_case("p2d_q1g3_n97_B3_value")(_poisson_case(_kw2(97, 3), 3, [("value", "obj"), ("f32", "box")], 50))
_case("p2d_q1g3_n65_B1_fgp")(_poisson_case(_kw2(65, 3), 1, [("u8", "box")], 60, force="fgp"))
_case("p2d_q2g3_n65_B3_u8")(_poisson_case(_kw2(65, 3, deg=2), 3, [("u8", "obj"), ("u8", "box")], 70))
_case("p2d_q2g4_n33_B1_fgp")(_poisson_case(_kw2(33, 4, deg=2), 1, [("f32", "box")], 80, force="fgp", residual=False))
# 3-D Poisson Q1: even x (the box / two-element path), odd x, nz - 1 no multiple of any strip height, a tiny mesh; BoxFaces alone and beside
# a mask image, the assembled load vector
_K3 = lambda n, ngp=2, sizes=None: dict(_kw2(n, ngp, sizes=sizes), nsd=3)
_case("p3d_g2_n34_B2_box")(_poisson_case(_K3(34), 2, [("box", "box")], 110))
_case("p3d_g2_n34_B1_box_obj")(_poisson_case(_K3(34), 1, [("u8", "obj"), ("box", "box")], 120))
_case("p3d_g2_34x21x11_B2_load")(_poisson_case(_K3(34, sizes=(34, 21, 11)), 2, [("u8", "box")], 130, force="load"))
_case("p3d_g2_34x21x11_B1_box_load")(_poisson_case(_K3(34, sizes=(34, 21, 11)), 1, [("box", "box")], 135, force="load"))
_case("p3d_g2_n33_B1_box_f32")(_poisson_case(_K3(33), 1, [("f32", "obj"), ("box", "box")], 140))
_case("p3d_g3_n17_B2_u8")(_poisson_case(_K3(17, 3), 2, [("u8", "obj"), ("u8", "box")], 150))
_case("p3d_g2_5x4x3_B1_box")(_poisson_case(_K3(5, sizes=(5, 4, 3)), 1, [("box", "box")], 160))
_case("p3d_g2_6x5x3_B3_box")(_poisson_case(_K3(6, sizes=(6, 5, 3)), 3, [("box", "box")], 165))


# ---- prepared launches: a pipelined chain of three with fold, a split evaluation, async sums ---------------------------------------
def _chain_case(kw, B, form, seed):
    def build():
        from diffnet_amd import ops
        m = module(kw)
        shape = (B, 1, *m.geom.node_shape)
        sets = [(seeded(shape, seed + 3 * k), seeded(shape, seed + 3 * k + 1, 0.5), seeded(shape, seed + 3 * k + 2)) for k in range(3)]
        dg, dr, _ = _conds(shape, [(form, "box")], seed)
        scale = 1.0 / (B * m.geom.nelem_total)
        kwargs = dict(alpha=2.0, beta=1.0, c=1.0, wscale=1.0, out_scale=scale, want_out=True, want_sums=True, loss_scale=scale)

        def gpu():
            plans = [ops.PoissonPlan(m.geom, *(t.to(dev()) for t in s), None, dg, pipelined_sums=True, **kwargs) for s in sets]
            for k in (1, 2):
                plans[k].fold(plans[k - 1])
            for p in plans:
                _sentinel(*p.result)
            for p in plans:
                p.launch()
            plans[2].finish_sums()
            res = {}
            for k, p in enumerate(plans):
                res.update({f"loss{k}": ("s", p.result[2]), f"energy{k}": ("s", p.result[1][0]), f"sumsq{k}": ("s", p.result[1][1]),
                            f"grad{k}": ("g", p.result[0])})
            return res

        def ref():
            o = _oracle(kw)
            out = {}
            for k, (u, nu, f) in enumerate(sets):
                ur = u.double().requires_grad_(True)
                e = o.energy(ur, nu.double(), f.double(), dirichlet=dr, c=1.0)
                (g,) = torch.autograd.grad(e, ur)
                out.update({f"loss{k}": _np(e), f"energy{k}": _np(e) / scale, f"sumsq{k}": float(np.sum(_np(g) ** 2)) / scale ** 2,
                            f"grad{k}": _np(g)})
            return out

        return gpu, ref
    return build


_case("fold2d_q1g3_n64_B2_u8")(_chain_case(_kw2(64, 3), 2, "u8", 200))
_case("fold2d_q1g3_72x45_B1_packed")(_chain_case(_kw2(72, 3, sizes=(72, 45)), 1, "packed", 210))
_case("fold3d_g2_n34_B2_u8")(_chain_case(_K3(34), 2, "u8", 220))
_case("fold3d_g2_34x21x11_B1_box")(_chain_case(_K3(34, sizes=(34, 21, 11)), 1, "box", 230))


def _split_case(kw, B, form, seed, async_sums=False):
    def build():
        from diffnet_amd import ops
        m = module(kw)
        shape = (B, 1, *m.geom.node_shape)
        u, nu, f = seeded(shape, seed), seeded(shape, seed + 1, 0.5), seeded(shape, seed + 2)
        dg, dr, _ = _conds(shape, [("u8", "obj"), (form, "box")], seed)
        scale = 1.0 / (B * m.geom.nelem_total)
        kwargs = dict(alpha=1.0, beta=1.0, c=0.5, wscale=1.0, out_scale=scale, want_out=True, want_sums=True, loss_scale=scale)

        def gpu():
            a = (u.to(dev()), nu.to(dev()), f.to(dev()), None, dg)
            if async_sums:
                p = ops.PoissonPlan(m.geom, *a, async_sums=True, **kwargs)
                _sentinel(*p.result)
                p.launch()
                p.wait_sums()
                out, sums, loss = p.result
            else:
                p1 = ops.PoissonPlan(m.geom, *a, strip_select=1, **kwargs)
                p2 = ops.PoissonPlan(m.geom, *a, strip_select=2, continues=p1, **kwargs)
                _sentinel(*p1.result)
                p1.launch()
                p2.launch()
                out, sums, loss = p1.result
            return dict(loss=("s", loss), energy=("s", sums[0]), sumsq=("s", sums[1]), grad=("g", out))

        def ref():
            ur = u.double().requires_grad_(True)
            e = _oracle(kw).energy(ur, nu.double(), f.double(), dirichlet=dr, c=0.5)
            (g,) = torch.autograd.grad(e, ur)
            return dict(loss=_np(e), energy=_np(e) / scale, sumsq=float(np.sum(_np(g) ** 2)) / scale ** 2, grad=_np(g))

        return gpu, ref
    return build


_case("split2d_q1g3_n130_B1_packed")(_split_case(_kw2(130, 3), 1, "packed", 300))
_case("split2d_q1g2_n65_B3_u8")(_split_case(_kw2(65, 2), 3, "u8", 310))
_case("split3d_g2_n34_B1_box")(_split_case(_K3(34), 1, "box", 320))
_case("async2d_q1g3_n64_B2_packed")(_split_case(_kw2(64, 3), 2, "packed", 330, async_sums=True))
_case("async3d_g2_n34_B1_u8")(_split_case(_K3(34), 1, "u8", 340, async_sums=True))


# ---- FSDT: one-shot residuals + norms, and the defer_norms -> norms_from pair (FsdtPlan) ---------------------------------------------
def _fsdt_case(n, deg, B, seed):
    def build():
        from diffnet_amd import ops
        from diffnet_amd.elasticity import _constants
        kw = dict(domain_size=n, fem_basis_deg=deg)
        m = module(kw)
        shape = (B, 1, n, n)
        flds = [seeded(shape, seed + i, -0.5) for i in range(3)]
        bc = boundary_mask(shape)
        E, v, th, Ks, q = 2.0, 0.3, 0.2, 5.0 / 6.0, 1.5
        consts, wscale = _constants(E, v, th, Ks), (0.5 * m.h) ** 2
        wts = [1.0, 0.5, 2.0]

        def gpu():
            fd = [t.to(dev()) for t in flds]
            bcd = bc.to(dev())
            outs, sums, norms = ops.fsdt_apply(m.geom, *fd, bcd, q=q, wscale=wscale, want_norms=True, **consts)
            plan = ops.FsdtPlan(m.geom, *fd, bcd, weights=wts, q=q, wscale=wscale, **consts)
            _sentinel(plan.residuals, plan.norms, plan.grads)
            pn, pg = plan.launch()
            torch.cuda.synchronize()
            res = {f"R{k}": ("f", outs[k]) for k in range(3)}
            res.update({f"sumsq{k}": ("s", sums[k]) for k in range(3)})
            res.update({f"norm{k}": ("s", norms[k]) for k in range(3)})
            res.update({f"plan_norm{k}": ("s", pn[k]) for k in range(3)})
            res.update({f"plan_grad{k}": ("g", pg[k]) for k in range(3)})
            return res

        def ref():
            o = _oracle(kw)
            ins = [t.double().requires_grad_(True) for t in flds]
            Rs = o.fsdt_residuals(*ins, bc.double(), E=E, v=v, th=th, Ks=Ks, q=q)
            nr = [torch.sqrt(torch.sum(R ** 2)) for R in Rs]
            gs = torch.autograd.grad(sum(w * x for w, x in zip(wts, nr)), ins)
            out = {f"R{k}": _np(Rs[k]) for k in range(3)}
            out.update({f"sumsq{k}": _np(nr[k]) ** 2 for k in range(3)})
            out.update({f"norm{k}": _np(nr[k]) for k in range(3)})
            out.update({f"plan_norm{k}": _np(nr[k]) for k in range(3)})
            out.update({f"plan_grad{k}": _np(gs[k]) for k in range(3)})
            return out

        return gpu, ref
    return build


_case("fsdt_q1_n33_B2")(_fsdt_case(33, 1, 2, 400))
_case("fsdt_q2_n33_B1")(_fsdt_case(33, 2, 1, 410))
_case("fsdt_q3_n34_B1")(_fsdt_case(34, 3, 1, 420))


# ---- gauss_pt_eval forward and adjoint, 2-D and 3-D ---------------------------------------------------------------------------------
def _gpe_case(kw, B, seed):
    def build():
        from diffnet_amd import gauss_pt_eval
        m = module(kw)
        nsd = kw.get("nsd", 2)
        o = _oracle(kw)
        shape = (B, 1, *m.geom.node_shape)
        x = seeded(shape, seed, -0.5)
        names = ["N_gp"] + ["dN_%s_gp" % a for a in "xyz"[:nsd]]
        G = m.geom.ngp_total
        cot = seeded((B, G, *m.geom.elem_shape), seed + 1, -0.5)
        stride = kw.get("fem_basis_deg", 1)

        def gpu():
            res = {}
            for n in names:
                T = o.t[n].float().reshape(G, -1).to(dev())
                xg = x.to(dev()).requires_grad_(True)
                y = gauss_pt_eval(xg, T, nsd=nsd, stride=stride)
                (gx,) = torch.autograd.grad(y, xg, cot.to(dev()))
                res.update({f"fwd_{n}": ("f", y), f"adj_{n}": ("f", gx)})
            return res

        def ref():
            out = {}
            for n in names:
                xr = x.double().requires_grad_(True)
                y = o.ev(xr, n)
                (gx,) = torch.autograd.grad(y, xr, cot.double())
                out.update({f"fwd_{n}": _np(y), f"adj_{n}": _np(gx)})
            return out

        return gpu, ref
    return build


_case("gpe2d_q1g3_n33_B2")(_gpe_case(_kw2(33, 3), 2, 500))
_case("gpe2d_q2g3_n31x20_B1")(_gpe_case(_kw2(31, 3, deg=2, sizes=(31, 21)), 1, 510))
_case("gpe3d_q1g2_n17_B2")(_gpe_case(_K3(17), 2, 520))
_case("gpe3d_q1g3_13x9x6_B1")(_gpe_case(_K3(13, 3, sizes=(13, 9, 6)), 1, 530))


# ---- conv2d 4 x 4 / stride 2: down / up / wrw against float64 torch convolutions ----------------------------------------------------
def _conv_case(B, C, M, H, W, seed):
    def build():
        import torch.nn.functional as F
        from diffnet_amd.networks.fused import _c2_down, _c2_up, _c2_wrw
        g = torch.Generator().manual_seed(seed)
        fine = torch.randn((B, C, 2 * H, 2 * W), generator=g)
        coarse = torch.randn((B, M, H, W), generator=g)
        w = torch.randn((M, C, 4, 4), generator=g) * 0.1

        def gpu():
            fd, cd, wd = fine.to(dev()), coarse.to(dev()), w.to(dev())
            return dict(down=("c", _c2_down(fd, wd)), up=("c", _c2_up(cd, wd)), wrw=("w", _c2_wrw(fd, cd)))

        def ref():
            fr, wr = fine.double().requires_grad_(True), w.double().requires_grad_(True)
            y = F.conv2d(fr, wr, None, 2, 1)
            gf, gw = torch.autograd.grad(y, (fr, wr), coarse.double())
            return dict(down=_np(y), up=_np(gf), wrw=_np(gw))

        return gpu, ref
    return build


_case("conv2d_B2_C8_M16_32x64")(_conv_case(2, 8, 16, 16, 32, 600))
_case("conv2d_B1_C48_M40_32x32")(_conv_case(1, 48, 40, 16, 16, 610))
_case("conv2d_ragged_B1_C3_M5_18x22")(_conv_case(1, 3, 5, 9, 11, 620))


# ---------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------
_BUILT, _REF, _BASE = {}, {}, {}


def _built(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def _ref(name):
    if name not in _REF:
        _REF[name] = _BUILT[name][1]()
    return _REF[name]


def _run(name):
    res = _built(name)[0]()
    torch.cuda.synchronize()
    return {k: (kind, _np(t)) for k, (kind, t) in res.items()}


def _check_oracle(name, got, ref, label):
    for k, (kind, a) in got.items():
        r = np.asarray(ref[k], dtype=np.float64).reshape(a.shape)
        msg = f"{name} [{label}] {k}"
        assert np.isfinite(a).all(), f"{msg}: non-finite values (an output left unwritten: sentinel NaN)"
        if kind in ("c", "w"):
            # (test_gpu_round4.py: 2e-5 of the largest magnitude, 4e-5 for weight gradients -- thousands of positions summed per weight in fp32)
            err = float(np.abs(a - r).max())
            tol = 4e-5 if kind == "w" else 2e-5
            assert err <= tol * (float(np.abs(r).max()) + 1e-30), f"{msg}: max error {err} against the float64 convolution"
        elif kind == "s":
            np.testing.assert_allclose(a, r, rtol=1e-5, err_msg=f"{msg} against the float64 oracle (sentinel -1: unwritten)")
        else:
            rt = 1e-4 if kind == "g" else 1e-5
            at = (1e-4 if kind == "g" else 1e-6) * max(1e-30, float(np.abs(r).max()))
            np.testing.assert_allclose(a, r, rtol=rt, atol=at, err_msg=f"{msg} against the float64 oracle")


def _base(name):
    if name not in _BASE:
        from diffnet_amd import _lib
        for key, _ in SETTINGS:
            assert _lib.config_get(key) == "", f"switch {key} is set outside this test"
        got = _run(name)
        _check_oracle(name, got, _ref(name), "default")
        _BASE[name] = got
    return _BASE[name]


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


def test_settings_cover_every_switch():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffnet_amd", "csrc", "dn_api.hip")).read()
    keys = re.search(r"kKeys\[[^\]]*\]\s*=\s*\{([^}]*)\}", src).group(1)
    keys = set(re.findall(r'"([A-Z0-9_]+)"', keys))
    assert keys - NOT_CROSSED == {k for k, _ in SETTINGS}
    for (k, v, pat), why in EXPECTED_REFUSALS.items():
        assert k in keys and why and any(fnmatch.fnmatch(c, pat) for c in CASES), (k, v, pat)


@pytest.mark.parametrize("name", sorted(CASES))
def test_default_setting_matches_oracle(name):
    _base(name)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("key,value", SETTINGS, ids=[f"{k}={v}" for k, v in SETTINGS])
def test_switch_matches_default_and_oracle(key, value, name, switch):
    from diffnet_amd._lib import DiffNetHipError
    base = _base(name)
    switch(key, value)
    why = _refusal_reason(key, value, name)
    try:
        got = _run(name)
    except DiffNetHipError as e:
        assert why is not None, f"{name} under {key}={value}: unlisted refusal ({e})"
        return
    assert why is None, f"{name} under {key}={value}: listed in EXPECTED_REFUSALS ({why}) but ran"
    _check_oracle(name, got, _ref(name), f"{key}={value}")
    for k, (kind, a) in got.items():
        b = base[k][1]
        msg = f"{name} {k} under {key}={value} against the default setting"
        if kind == "s":
            np.testing.assert_allclose(a, b, rtol=2e-6, err_msg=msg)
        elif kind == "w":
            # a weight gradient sums B * H * W products per entry in K-slices whose split CONV_WRW_WGS / CONV2D_V1 choose: another order
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-5 * float(np.abs(b).max()), err_msg=msg)
        else:
            np.testing.assert_allclose(a, b, rtol=0, atol=2e-6 * max(1e-30, float(np.abs(b).max())), err_msg=msg)
