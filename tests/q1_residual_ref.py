"""What test_gpu_q1_residual_forms.py needs and no GPU: the argument sets of the four fused Q1 residual operators (stokes_apply, ns_apply,
transport_apply, poisson_coef_grad) as plain numpy data, a Python mirror of the host's kernel selection and of flow2d_plan
(csrc/flow2d_common.h), the float64 references with their per-node scale, the comparator and the per-family yardstick.

The reference of every operator is the restatement its host test file keeps (stokes_np, ns_torch, ns_vjp_np, transport_torch,
transport_vjp_np, restate), evaluated in float64 on the float32 values the kernel reads: fields, masks, forcing, constants (all chosen
exactly representable: the spacings are powers of two) and the 1-D tables as the mesh struct stores them (float32; the rules of 3 and 4
points are the reference's truncated literals, 1e-6 away from the exact Gauss points, so the restatements' own leggauss tables would not
do).  With `scale=True` a restatement also returns S, the sum of |w_g t| over the placed terms that make up a node's value.  A result is
judged node by node: e = |got - ref64| / S on the free nodes (S == 0: exactly 0), exact values on the Dirichlet nodes.  The bound is
K = MARGIN * Y, Y (the yardstick) being the largest e the float32 evaluation of the same restatement reaches over all the cases of the
family: it is measured against the reference alone."""
import collections
import functools
import itertools
import math
import zlib

import numpy as np
import torch

U = 2.0 ** -24                      # unit roundoff of float32
MARGIN = 4                          # a fused route over a reference route's own distance to float64 (test_strongform_fused_matches_composed)
HX, HY, HZ = 0.125, 0.25, 0.25      # powers of two: 2 / h, 4 / h^2 and their products are exact in float32
OWNERS = 62                         # owner columns of a wave (FLOW2D_OWNERS)
WS_HEADER = 64 * 65                 # DN_WS_HEADER (csrc/dn_reduce.h)
MIN_ROWS = dict(stokes=4, ns=8, transport=8, coef2d=8)
WS_DOUBLES = dict(stokes=3, ns=3, transport=1)
FAMILIES = ("stokes", "stokes_t", "ns", "ns_vjp", "transport", "transport_vjp", "coef2d", "coef3d")
OPERATOR = dict(stokes="stokes", stokes_t="stokes", ns="ns", ns_vjp="ns", transport="transport", transport_vjp="transport", coef2d="coef2d",
                coef3d="coef3d")
MESH1, MESH1_3D = (64, 10, 2), ((65, 4, 3), 2)          # part 1: a chunk seam and a strip seam; the 3-D block decode crosses 64 columns
# part 2: (nx, ny, B); what each reaches is asserted by test_seam_list_reaches_every_seam
SEAMS = [(2, 2, 1), (3, 9, 1), (62, 9, 2), (63, 25, 1), (64, 17, 3), (124, 15, 1), (125, 26, 2), (3, 57, 1), (2, 64, 600)]
NREF = 4                            # samples of a large batch that have inputs of their own: sample b repeats sample b % NREF

STOKES_C = dict(visco=0.75, pspg=0.03125, J=0.0625)
NS_C = dict(visco=0.0625, J=0.0625, tau_h=(HX, HY), cinv=36.0)
TRANSPORT_C = dict(adv=(0.75, -0.5), kappa=(0.0625, 0.03125), tau=0.046875, J=0.0625)
REACT = {False: (0.25, 0.0, 0.0, 0.0), True: (-0.75, 8.0, -24.0, 16.0)}
COEF_C = dict(a_nu=0.5, a_f=-0.75, wscale=0.25, in_scale=-2.5)

Spec = collections.namedtuple("Spec", "family ngp mesh B form i")        # form: a tuple of the host's selectors as the arguments set them


# ---------------------------------------------------------------------------------------------
# the launch plan (flow2d_plan) and the seams
# ---------------------------------------------------------------------------------------------
def plan(nx, ny, B, min_rows):
    chunks = -(-nx // OWNERS)
    per_row = chunks * B
    by_batch, by_rows = -(-4096 // per_row), -(-ny // min_rows)
    strips = max(min(by_batch, by_rows), 1)
    R = -(-ny // strips)
    strips = -(-ny // R)
    waves = chunks * strips
    wpb = min(waves, 4)
    gx = -(-waves // wpb)
    return dict(chunks=chunks, strips=strips, R=R, last=ny - (strips - 1) * R, wpb=wpb, gx=gx, idle=gx * wpb - waves,
                last_owners=nx - (chunks - 1) * OWNERS, batch_limited=by_batch < by_rows)


def seam_rows(ny, B, nx):
    """the node rows on both sides of every strip boundary of both plans (shortest strips of 4 and of 8 rows)"""
    rows = set()
    for mr in (4, 8):
        g = plan(nx, ny, B, mr)
        for s in range(1, g["strips"]):
            rows |= {s * g["R"] - 1, s * g["R"]}
    return sorted(r for r in rows if 0 <= r < ny)


# ---------------------------------------------------------------------------------------------
# seeded data
# ---------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def rnd(shape, *key, lo=-0.5, width=1.0):
    return (lo + width * _rng(*key).random(shape)).astype(np.float32)


def mask_image(node_shape, Bm, B, kind, *key, thr=False):
    """(Bm, *node_shape): a 20 % blob per sample plus, in 2-D, nodes on both sides of each seam -- of columns 61, 62 and 63 two of every
    three rows are fixed and the third is free, of the rows around each strip boundary one of every four columns is fixed and one is free
    (the same rows and columns for every condition of a case, so that some stay free under all of them).  kind "f32": 0 / 1 (thr: a few
    nodes take exactly 0.5 and its two float32 neighbours instead), "u8": 0 / 1 / 255.  key: (the case, the condition)."""
    rs = _rng("mask", *key)
    m = rs.random((Bm, *node_shape)) < 0.2
    if len(node_shape) == 2:
        ny, nx = node_shape
        off = int(_rng("offset", *key[:-1]).integers(0, 12))
        for r in seam_rows(ny, B, nx):
            m[:, r, (np.arange(nx) + r + off) % 4 == 0] = True
            m[:, r, (np.arange(nx) + r + off) % 4 == 2] = False
        for c in (61, 62, 63):
            if c < nx:
                m[:, (np.arange(ny) + c + off) % 3 != 0, c] = True
                m[:, (np.arange(ny) + c + off) % 3 == 0, c] = False
    if kind == "u8":
        return np.where(m, np.where(rs.random(m.shape) < 0.5, 255, 1), 0).astype(np.uint8)
    img = m.astype(np.float32)
    if thr:
        edge = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))], dtype=np.float32)
        pick = rs.random(m.shape) < 0.3
        img = np.where(pick, edge[rs.integers(0, 3, m.shape)], img).astype(np.float32)
    return img


def fixed_nodes(m, coef=False):
    """the Dirichlet nodes of a mask image as include/diffnet_hip.h states them: uint8 != 0; fp32 >= 0.5 (dn_stokes_args, dn_ns_args,
    dn_transport_args) or > 0.5 (dn_dirichlet: dn_coef_grad_args)"""
    if m is None:
        return None
    if m.dtype == np.uint8:
        return m != 0
    return (m > np.float32(0.5)) if coef else (m >= np.float32(0.5))


def pick(a, b):
    """sample b of a shared (leading 1) or per-sample array; a constant as it is"""
    return a[b if a.shape[0] > 1 else 0] if isinstance(a, np.ndarray) else a


def _nodal(node_shape, B, batched, *key, **kw):
    return rnd((B if batched else 1, *node_shape), *key, **kw)


# ---------------------------------------------------------------------------------------------
# the argument sets
# ---------------------------------------------------------------------------------------------
KINDS3 = [("f32", "u8", None), ("f32", "f32", "f32"), ("u8", None, "u8"), (None, "f32", "u8")]
KINDS2 = [("f32", "u8"), ("u8", None), (None, "f32"), ("f32", "f32"), ("u8", "u8")]


def part1_specs(family, ngp):
    """the full product of the host's remaining selectors, as argument sets, on the part-1 mesh"""
    if family == "coef3d":
        sizes, B = MESH1_3D
        return [Spec(family, ngp, sizes, B, f, i) for i, f in enumerate(itertools.product((False, True), (3,), range(5)))]
    mesh, B = MESH1[:2], MESH1[2]
    if family in ("stokes", "stokes_t", "ns", "ns_vjp"):
        forms = itertools.product(range(3), (False, True))                                   # sel, FGP
    elif family in ("transport", "transport_vjp"):
        forms = itertools.product((False, True), (False, True), range(3), (False, True))     # NU, REACT, sel, FGP
    else:
        forms = itertools.product((False, True), (1, 2, 3), range(5))                        # HASV, WANT, form
    return [Spec(family, ngp, mesh, B, f, i) for i, f in enumerate(forms)]


def part2_forms(family):
    if family in ("stokes", "stokes_t", "ns", "ns_vjp"):
        return [(2, True), (0, False), (1, True)]
    if family in ("transport", "transport_vjp"):
        return [(True, True, 2, True), (False, False, 0, False), (True, False, 1, False)]
    return [(True, 3, 4), (False, 3, 0), (True, 1, 1)]


def part2_specs(family):
    """every seam mesh with three forms: everything, nothing, and one between; the rule rotates with the mesh"""
    if family == "coef3d":
        return []
    return [Spec(family, 2 + (k + j) % 3, (nx, ny), B, f, 100 + 3 * k + j)
            for k, (nx, ny, B) in enumerate(SEAMS) for j, f in enumerate(part2_forms(family))]


def threshold_specs(family):
    """one masked case per operator whose fp32 masks hold 0.5 and its two neighbours (form: the masked one with value fields, "thr")"""
    if family == "coef3d":
        return [Spec(family, 2, MESH1_3D[0], MESH1_3D[1], (True, 3, 4, "thr"), 201)]
    return [Spec(family, 3, MESH1[:2], MESH1[2], (*part2_forms(family)[0], "thr"), 200)]


def all_specs(family):
    return [s for ngp in (2, 3, 4) for s in part1_specs(family, ngp)] + part2_specs(family) + threshold_specs(family)


def _conditions(n, kinds, sel, node_shape, B, i, key, thr, Bplan):
    """masks and values of n conditions: sel 0 none, 1 constants, 2 at least one value field; shared and per sample mixed by i"""
    masks, vals = [None] * n, [0.0] * n
    if sel == 0:
        return masks, vals
    consts = (0.3125, -0.25, 0.125)
    first_field = True
    for k in range(n):
        kind = "f32" if (thr and kinds[k] is not None) else kinds[k]
        if kind is None:
            continue
        masks[k] = mask_image(node_shape, B if (i + k) % 2 == 0 else 1, Bplan, kind, *key, k, thr=thr)
        vals[k] = consts[k]
        if sel == 2 and (first_field or (i + k) % 3 == 0):
            vals[k] = _nodal(node_shape, B, (i + k) % 2 == 1, *key, "val", k)
            first_field = False
    return masks, vals


def _tile(a, B):
    """a per-sample array of NREF samples repeated to B samples (sample b: b % NREF); shared arrays and constants as they are"""
    if isinstance(a, np.ndarray) and a.shape[0] == NREF:
        return np.ascontiguousarray(a[np.arange(B) % NREF])
    return a


@functools.lru_cache(maxsize=None)
def build(spec):
    """the argument set of a spec: numpy float32 / uint8 arrays and Python floats, named as the operator's Python entry names them"""
    family, ngp, mesh, B, form, i = spec
    thr = form[-1] == "thr"
    form = form[:-1] if thr else form
    Bb = min(B, NREF)                                   # samples with inputs of their own
    key = (family, ngp, mesh, B, form, i)
    G = ngp ** len(mesh)
    node_shape, elem_shape = tuple(mesh[::-1]), tuple(n - 1 for n in mesh[::-1])
    c = dict(spec=spec, family=family, ngp=ngp, mesh=mesh, B=B, nref=Bb, node_shape=node_shape)
    if family in ("stokes", "stokes_t", "ns", "ns_vjp"):
        sel, fgp = form
        c["fields"] = [rnd((Bb, *node_shape), *key, "fld", k, lo=-1.0, width=2.0) for k in range(3)]
        if family == "ns_vjp":
            c["cot"] = [rnd((Bb, *node_shape), *key, "cot", k) for k in range(3)]
        c["masks"], c["vals"] = _conditions(3, KINDS3[i % 4], sel, node_shape, Bb, i, key, thr, B)
        if fgp:
            which = ((True, True), (True, False), (False, True))[i % 3]              # one of the two may stay a constant
            c["f"] = [rnd((Bb if (i + k) % 2 == 0 else 1, G, *elem_shape), *key, "f", k) if which[k] else (0.375, 0.0)[k] for k in range(2)]
        else:
            c["f"] = [0.5, -0.25] if i % 2 else [0.0, 0.0]
    elif family in ("transport", "transport_vjp"):
        nu, react, sel, fgp = form
        c["u"] = rnd((Bb, *node_shape), *key, "u", lo=-1.0, width=2.0)
        if family == "transport_vjp":
            c["cot"] = rnd((Bb, *node_shape), *key, "cot")
        c["nu"] = _nodal(node_shape, Bb, i % 2 == 0, *key, "nu", lo=0.5) if nu else None
        c["masks"], c["vals"] = _conditions(2, KINDS2[i % 5], sel, node_shape, Bb, i, key, thr, B)
        c["f"] = rnd((Bb if (i // 2) % 2 == 0 else 1, G, *elem_shape), *key, "f", width=4.0, lo=-2.0) if fgp else (0.625 if i % 3 else 0.0)
        c["react"], c["first"] = REACT[react], bool((i // 2) % 2)
    else:
        hasv, want, frm = form
        c["u"] = rnd((Bb, *node_shape), *key, "u", lo=-1.0, width=2.0)
        c["v"] = rnd((Bb, *node_shape), *key, "v") if hasv else None
        nbc = 0 if frm == 0 else 1 + i % 2
        kind = "u8" if (frm in (1, 3) and not thr) else "f32"
        c["masks"], c["vals"] = _conditions(nbc, (kind,) * nbc, 0 if frm == 0 else (2 if frm >= 3 else 1), node_shape, Bb, i, key, thr, B)
        if frm >= 3 and nbc == 2 and i % 4 == 1:               # the field on the second condition alone
            c["vals"] = [0.3125, _nodal(node_shape, Bb, True, *key, "val", 1)]
        c["want"] = tuple(n for n, bit in (("nu", 1), ("f", 2)) if want & bit)
        c["in_scale"] = COEF_C["in_scale"] if i % 2 else None
    if B > Bb:
        for k, v in list(c.items()):
            c[k] = [_tile(x, B) for x in v] if isinstance(v, list) else _tile(v, B)
    return c


# ---------------------------------------------------------------------------------------------
# the host's kernel selection, mirrored
# ---------------------------------------------------------------------------------------------
def _is_field(x):
    return isinstance(x, np.ndarray)


def selectors(c):
    """the template arguments the host picks for an argument set (the rules quoted in the issue from stokes.hip, navier_stokes.hip,
    flow2d_common.h flow2d_launch, transport.hip:315-353 and poisson_coef_grad.hip:456-459), NGP first"""
    fam, ngp = c["family"], c["ngp"]
    mask = any(m is not None for m in c["masks"])
    if fam in ("stokes", "stokes_t", "ns", "ns_vjp"):
        tr = fam == "stokes_t"                              # the transpose launch drops the value fields and the forcing
        bcf = (not tr) and any(_is_field(v) for v in c["vals"])
        fgp = (not tr) and any(_is_field(f) for f in c["f"])
        sel = (2 if bcf else 1) if mask else 0
        if fam in ("stokes", "stokes_t"):
            return (ngp if fgp else 2, sel, fgp)            # stokes.hip:203: without Gauss-point forcing one kernel serves every rule
        return (ngp, sel, fgp, fam == "ns_vjp")
    if fam in ("transport", "transport_vjp"):
        vjp = fam == "transport_vjp"
        react = any(x != 0.0 for x in c["react"][1:])
        needu = (not vjp) or react
        bcf = needu and any(_is_field(v) for v in c["vals"])
        sel = (2 if bcf else 1) if mask else 0
        return (ngp, c["nu"] is not None, react, sel, (not vjp) and _is_field(c["f"]), vjp)
    want = (1 if "nu" in c["want"] else 0) | (2 if "f" in c["want"] else 0)
    hasv = c["v"] is not None
    needu = bool(want & 1) or not hasv
    form = 0 if not mask else (1 if c["masks"][0].dtype == np.uint8 else 2)
    if form and any(_is_field(v) for v in c["vals"]) and (needu or fam == "coef3d"):
        form += 2
    return (ngp, hasv, want, form) if fam == "coef2d" else (ngp, hasv, form)


def expected_kernels(family, ngp):
    """the instantiations the dispatch can pick for one operator, mode and rule"""
    if family == "stokes":
        return {(ngp if fgp else 2, sel, fgp) for sel in range(3) for fgp in (False, True)}
    if family == "stokes_t":
        return {(2, sel, False) for sel in range(2)}
    if family in ("ns", "ns_vjp"):
        return {(ngp, sel, fgp, family == "ns_vjp") for sel in range(3) for fgp in (False, True)}
    if family == "transport":
        return {(ngp, nu, react, sel, fgp, False) for nu in (False, True) for react in (False, True) for sel in range(3) for fgp in (False, True)}
    if family == "transport_vjp":
        return {(ngp, nu, react, sel, False, True) for nu in (False, True) for react in (False, True) for sel in range(3 if react else 2)}
    if family == "coef2d":
        return {(ngp, hasv, want, form) for hasv in (False, True) for want in (1, 2, 3) for form in range(5 if (want & 1 or not hasv) else 3)}
    return {(ngp, hasv, form) for hasv in (False, True) for form in range(5)}


# ---------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables_f32(ngp):
    """the 1-D tables (N, dN, w) as dn_mesh carries them: the reference's rule and basis, rounded to float32"""
    from diffnet_amd.tables import Basis1D, gauss_rule
    gx, gw = gauss_rule(ngp)
    Bv, Dv, _ = Basis1D(1).at_gauss(gx)
    return tuple(np.asarray(t, dtype=np.float32) for t in (Bv, Dv, gw))


@functools.lru_cache(maxsize=None)
def _oracle(mesh, ngp):
    from test_coef_grad_host import oracle64
    nsd = len(mesh)
    hs = (HX, HY, HZ)
    return oracle64(nsd=nsd, domain_sizes=tuple(mesh) + (1,) * (3 - nsd), domain_lengths=tuple((n - 1) * h for n, h in zip(tuple(mesh) + (2,) * (3 - nsd), hs)),
                    ngp_1d=ngp)


def _full(f, b, G, elem_shape):
    f = pick(f, b)
    return f if isinstance(f, np.ndarray) else np.full((G, *elem_shape), f, dtype=np.float32)


def evaluate(c, single=False, swap_scales=False):
    """The restatement of the case's operator on the case's float32 values, per sample with inputs of its own.  Returns a list with one
    entry per output: dict(name, ref, S, fixed, exact) -- (nref, *node_shape) arrays: the values (float64, or float32 with `single`), the
    scale, the Dirichlet nodes of the output and the exact values they must hold.  swap_scales: a deliberately wrong evaluation, the x and
    y derivative scales exchanged (2-D flow and transport operators; test_comparator_has_teeth)."""
    hx, hy = (HY, HX) if swap_scales else (HX, HY)
    from test_coef_grad_host import restate
    from test_ns_host import ns_torch, ns_vjp_np
    from test_stokes_host import stokes_np
    from test_transport_host import transport_torch, transport_vjp_np
    fam, ngp, nref, shape = c["family"], c["ngp"], c["nref"], c["node_shape"]
    npd, td = (np.float32, torch.float32) if single else (np.float64, torch.float64)
    if fam in ("coef2d", "coef3d"):
        o = _oracle(c["mesh"], ngp)
        t4 = lambda a: torch.from_numpy(np.ascontiguousarray(a[:nref] if a.shape[0] > 1 else a)).unsqueeze(1)      # noqa: E731
        dl = [(t4(m).double(), t4(v).double() if _is_field(v) else v) for m, v in zip(c["masks"], c["vals"])]
        s = 1.0 if c["in_scale"] is None else c["in_scale"]
        out = restate(o, t4(c["u"]).double(), None if c["v"] is None else t4(c["v"]).double(), dl, COEF_C["a_nu"] * s, COEF_C["a_f"] * s,
                      COEF_C["wscale"], scale=True, dtype=td)
        res = []
        for k, n in enumerate(("nu", "f")):
            if n in c["want"]:
                ref, S = out[k][:, 0].numpy(), out[2 + k][:, 0].numpy()
                res.append(dict(name="g_" + n, ref=ref, S=S, fixed=np.zeros(ref.shape, bool), exact=np.zeros(ref.shape, np.float32)))
        return res
    tabs = tables_f32(ngp)
    G, eshape = ngp * ngp, (shape[0] - 1, shape[1] - 1)
    nout = 1 if fam.startswith("transport") else 3
    acc = [dict(name=f"out{k}", ref=[], S=[], fixed=[], exact=[]) for k in range(nout)]
    for b in range(nref):
        masks = [fixed_nodes(pick(m, b)) if m is not None else None for m in c["masks"]]
        vals = [pick(v, b) for v in c["vals"]]
        vals32 = [np.broadcast_to(np.float32(v), shape) for v in vals]
        if nout == 3:
            flds = [f[b] for f in c["fields"]]
            f1, f2 = (_full(f, b, G, eshape) for f in c["f"])
            fx = [np.zeros(shape, bool) if m is None else m for m in masks]
            if fam == "stokes":
                R, S = stokes_np(*flds, masks, vals, f1, f2, hx=hx, hy=hy, ngp=ngp, scale=True, dtype=npd, tables=tabs, **STOKES_C)
                ex = vals32
            elif fam == "stokes_t":        # J_R^T = S J_R S, S = diag(1, 1, -1), the form test_stokes_host.py proves; zero values, no forcing
                zero = np.zeros((G, *eshape), np.float32)
                R, S = stokes_np(flds[0], flds[1], -flds[2], masks, [0.0] * 3, zero, zero, hx=hx, hy=hy, ngp=ngp, scale=True, dtype=npd, tables=tabs,
                                 **STOKES_C)
                R = (R[0], R[1], -R[2])
                ex = [np.zeros(shape, np.float32)] * 3
            elif fam == "ns":
                R, S = ns_torch(*[torch.from_numpy(f) for f in flds], masks, vals, f1, f2, hx=hx, hy=hy, ngp=ngp, scale=True, dtype=td, tables=tabs, **NS_C)
                R, S = [r.numpy() for r in R], [s.numpy() for s in S]
                ex = vals32
            else:
                R, S = ns_vjp_np(*flds, [t[b] for t in c["cot"]], masks, vals, f1, f2, hx=hx, hy=hy, ngp=ngp, scale=True, dtype=npd, tables=tabs, **NS_C)
                ex = [np.zeros(shape, np.float32)] * 3
        else:
            m0, m1 = (np.zeros(shape, bool) if m is None else m for m in masks)
            kw = dict(nu=None if c["nu"] is None else pick(c["nu"], b), masks=masks, vals=vals, f=pick(c["f"], b), react=c["react"], hx=hx, hy=hy, ngp=ngp,
                      first=c["first"], scale=True, tables=tabs, **TRANSPORT_C)
            fx = [m0 | m1]
            if fam == "transport":
                R, S = transport_torch(torch.from_numpy(c["u"][b]), dtype=td, **kw)
                R, S = [R.numpy()], [S.numpy()]
                order = (1, 0) if c["first"] else (0, 1)            # the condition applied last wins on the rows of R
                e = np.zeros(shape, np.float32)
                for k in order:
                    e = np.where((m0, m1)[k], vals32[k], e)
                ex = [e]
            else:
                R, S = transport_vjp_np(c["u"][b], c["cot"][b], dtype=npd, **kw)
                R, S, ex = [R], [S], [np.zeros(shape, np.float32)]
        for k in range(nout):
            assert R[k].dtype == npd, (fam, R[k].dtype)
            for n, x in (("ref", R[k]), ("S", S[k]), ("fixed", fx[k]), ("exact", ex[k])):
                acc[k][n].append(np.asarray(x))
    return [dict(name=a["name"], **{n: np.stack(a[n]) for n in ("ref", "S", "fixed", "exact")}) for a in acc]


@functools.lru_cache(maxsize=None)
def reference(spec):
    """float64 values, scale, Dirichlet nodes and their exact values: computed once per session and left unchanged"""
    out = evaluate(build(spec))
    for o in out:
        for a in o.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------
def node_error(got, o, strict=True):
    """e = |got - ref64| / S per node.  inf where a rule is broken: a non-finite value, a free node without a term (S == 0) that is not
    exactly 0, a Dirichlet node that does not hold its exact value.  Returns (max e, its index).  strict=False leaves the free nodes with
    S == 0 out: the yardstick's float32 evaluation adds a constant's four corner products in an order that need not cancel (the gradient
    of a constant Dirichlet patch in g_nu), which says nothing about the distance to float64 where there is a scale."""
    got32 = np.asarray(got)
    got = got32.astype(np.float64)
    ref, S, fixed = o["ref"].astype(np.float64), o["S"].astype(np.float64), o["fixed"]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    pos = S > 0
    e = np.where(pos, np.abs(got - ref) / np.where(pos, S, 1.0), np.where((got == 0.0) | (not strict), 0.0, math.inf))
    e = np.where(fixed, np.where(got32.astype(np.float32) == o["exact"], 0.0, math.inf), e)
    e = np.where(np.isfinite(got), e, math.inf)
    at = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[at]), tuple(int(x) for x in at)


def sums_bound(o, K, R, weight=None):
    """(sum of ref64^2, its bound): the kernels add r^2 in fp32 per lane over a strip of R rows, then reduce in fp64, so
    |got - sum ref64^2| <= 2 K sum |ref64| S + (R + 2) 2^-24 sum ref64^2.  weight: how often each sample counts."""
    ref, S = o["ref"].astype(np.float64), o["S"].astype(np.float64)
    w = np.ones(ref.shape[0]) if weight is None else np.asarray(weight, dtype=np.float64)
    w = w.reshape((-1,) + (1,) * (ref.ndim - 1))
    total = float((w * ref * ref).sum())
    return total, 2.0 * K * float((w * np.abs(ref) * S).sum()) + (R + 2) * U * total


@functools.lru_cache(maxsize=None)
def yardstick(family):
    """Y: the largest e of the float32 CPU evaluation of the restatement over every case of the family in this file; (Y, the case)"""
    worst, where = 0.0, None
    for spec in all_specs(family):
        ref = reference(spec)
        for o, s in zip(ref, evaluate(build(spec), single=True)):
            assert s["ref"].dtype == np.float32
            e, at = node_error(s["ref"], o, strict=False)
            assert math.isfinite(e), (spec, o["name"], at)
            if e > worst:
                worst, where = e, (spec, o["name"], at)
    return worst, where
