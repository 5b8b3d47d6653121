"""What test_gpu_elem2d_forms.py needs and no GPU: the argument sets of the four element-march operators (strongform_apply, fosls_apply,
helmholtz_apply, eikonal_apply and its VJP) as plain numpy data, a Python mirror of the host's kernel selection (elem2d_launch,
elem2d_launch_forms, elem2d_launch_mask and the four Family::launch) and of elem2d_plan (csrc/elem2d_common.h), the float64 references
with their magnitude field, the comparator, the sum bounds and the per-family yardstick.

The reference of every operator is the restatement its host test file keeps (strongform_np, fosls_np, helmholtz_np, eikonal_t64,
eikonal_pullback_np), evaluated in float64 on the float32 values the kernel reads: fields, masks, forcing, the constants (all short dyadic
numbers; the spacings are powers of two, so (float)(d * 2/h) and (float)(d2 * (2/h)^2) are exact) and the 1-D tables as the mesh struct
stores them (float32), with the weights formed as elem2d_fill forms them.  With `scale=True` a restatement also returns the magnitude
field S: the same formula with every input, table entry and constant replaced by its absolute value and every subtraction made an
addition, after the Dirichlet substitutions, 0 where the operator writes 0.  A result is judged node by node: e = |got - ref64| / S on the
free nodes (S == 0: exactly 0), exactly 0 on the Dirichlet nodes of an output that has them.  The bound is K = MARGIN * Y, Y (the
yardstick) being the largest e the float32 evaluation of the same restatement reaches over all the cases of the family and mode: it is
measured against the reference alone."""
import collections
import functools
import itertools
import math

import numpy as np
import torch

from q1_residual_ref import MARGIN, NREF, U, _rng, _tile, node_error, pick, rnd, sums_bound      # noqa: F401  (re-exported)

HX, HY = 0.125, 0.25                # powers of two and different: 2 / h and (2 / h)^2 are exact in float32
FAMILIES = ("strongform", "fosls", "helmholtz", "eikonal", "eikonal_vjp")          # family and mode
DEGREE_RULES = [(1, 2), (1, 3), (1, 4), (2, 3), (2, 4), (3, 3), (3, 4)]            # the switch of elem2d_launch
MESH1, PLAN1 = (65, 6, 2), "64,4"   # part 1 (nelx, nely, B): two chunks with a hand-over column, strips of 4 + 2 element rows
# part 2: (nelx, nely, B, plan), "" the default plan; what each reaches is asserted by test_seam_list_reaches_every_property.  The last
# one is not in the issue's table: two chunks of two waves each, which none of the table's 128- and 192-thread cases has
SEAMS = [(1, 1, 1, ""), (62, 3, 1, "64,4"), (63, 4, 2, "64,4"), (64, 5, 1, ""), (64, 5, 1, "64,4"), (126, 7, 2, "64,1"), (127, 7, 1, "64,3"),
         (127, 9, 3, "128,4"), (130, 9, 1, "192,2"), (255, 2, 1, "256,64"), (256, 2, 1, ""), (2, 33, 1, ""), (2, 2, 600, ""), (200, 3, 1, "128,2")]
SEAM_RULES = [(1, 2), (2, 3), (3, 4)]

WSCALE, OUT_SCALE, IN_SCALE = 0.25, 0.5, -2.0
SF_C = dict(ax=0.5, ay=-0.25, b=0.75, fs=0.75, d2=[(-0.0625, 0.03125), (0.0625, 0.0), (0.0, -0.03125)])
FO_C = dict(weights=(0.75, 0.5), fs=1.5, nu=0.625)
HH_C = dict(ecoef=(0.5, 0.375, 0.75), ocoef=(1.0, 0.75, 1.25), sigma=2.5)
EK_C = dict(tau=0.25, sq=1.25)
NAMES = dict(strongform=["grad"], fosls=["g_u", "g_mx", "g_my"], helmholtz=["out"], eikonal=["R"], eikonal_vjp=["vjp"])       # the output fields
IN_NUM, IN_DEN = 0.5, 2.0           # the VJP's scale of the cotangent: 0.25, exact

# form: (FK, M, *own) -- FK 0 | 1 | 2 (forcing: constant, nodal, at the Gauss points), M 0 | 1 | 2 (no condition, conditions with constant
# values, a value field), own: strong-form (NL, D2), FOSLS (NUF,), Helmholtz (CF,), eikonal ()
Spec = collections.namedtuple("Spec", "family P ngp nelx nely B plan form i")


# ---------------------------------------------------------------------------------------------
# the launch plan (elem2d_plan) and the seams
# ---------------------------------------------------------------------------------------------
def plan(P, nx, ny, B, override=""):
    """elem2d_plan: threads per workgroup by utilisation of the last chunk, then the strip height; "T,R" overrides both"""
    Q, nely = (nx - 1) // P + 1, (ny - 1) // P
    chunks_of = lambda T: 1 if Q <= T else -(-(Q - 1) // (T - 1))                # noqa: E731
    best, T, chunks = -1.0, 64, 1
    for t in (64, 128, 192, 256):
        score = Q / (chunks_of(t) * t) + 0.0003 * t
        if score > best:
            best, T, chunks = score, t, chunks_of(t)
    per_strip = chunks * B * (T // 64)
    R = 32
    while R > 4 and per_strip * -(-nely // R) < 4096:
        R //= 2
    if override:
        t, r = (int(x) for x in override.split(","))
        if 64 <= t <= 256 and t % 64 == 0 and r >= 1:
            T, R, chunks = t, r, chunks_of(t)
    R = max(1, min(R, nely))
    strips = -(-nely // R)
    used = Q - (chunks - 1) * (T - 1)               # thread columns of the last chunk that lie on the mesh (the closing column is one)
    return dict(T=T, chunks=chunks, R=R, strips=strips, last=nely - (strips - 1) * R, used=used, waves=T // 64, Q=Q)


def seam_nodes(P, nx, ny, B, override):
    """(node rows, node columns) on both sides of every strip and chunk boundary of the override's plan and of the default plan, and
    the last row and column, which the closing thread column and the closing emit own"""
    rows, cols = {ny - 1}, {nx - 1}
    for ov in {override, ""}:
        g = plan(P, nx, ny, B, ov)
        for s in range(1, g["strips"]):
            rows |= {s * g["R"] * P + d for d in (-1, 0, 1)}
        for c in range(1, g["chunks"]):
            cols |= {c * (g["T"] - 1) * P + d for d in (-1, 0, 1)}
    return sorted(r for r in rows if 0 <= r < ny), sorted(c for c in cols if 0 <= c < nx)


# ---------------------------------------------------------------------------------------------
# seeded data
# ---------------------------------------------------------------------------------------------
HALF = np.float32(0.5)
BELOW, ABOVE = np.nextafter(HALF, np.float32(0)), np.nextafter(HALF, np.float32(1))


def mask_image(node_shape, Bm, seams, kind, *key, thr=False):
    """(Bm, ny, nx): a 20 % blob per sample plus nodes on both sides of each seam -- of the seam columns two of every three rows are fixed
    and the third is free, of the seam rows one of every four columns is fixed and one is free, two of the four corners are fixed (the
    same rows, columns and corners for both conditions of a case, so that they overlap and some nodes stay free under both).  kind
    "f32": 0 / 1 (thr: a third of the nodes take a value at the threshold instead -- the fixed ones the float32 above 0.5, the free ones
    exactly 0.5 or the float32 below it: `> 0.5`, include/diffnet_hip.h), "u8": 0 / 1 / 255.  key: (the case, the condition)."""
    rs = _rng("mask", *key)
    ny, nx = node_shape
    m = rs.random((Bm, ny, nx)) < 0.2
    off = int(_rng("offset", *key[:-1]).integers(0, 12))
    rows, cols = seams
    for r in rows:
        m[:, r, (np.arange(nx) + r + off) % 4 == 0] = True
        m[:, r, (np.arange(nx) + r + off) % 4 == 2] = False
    for c in cols:
        m[:, (np.arange(ny) + c + off) % 3 != 0, c] = True
        m[:, (np.arange(ny) + c + off) % 3 == 0, c] = False
    for k, (j, i) in enumerate(((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1))):
        m[:, j, i] = (off + k) % 2 == 0
    if kind == "u8":
        return np.where(m, np.where(rs.random(m.shape) < 0.5, 255, 1), 0).astype(np.uint8)
    img = m.astype(np.float32)
    if thr:
        near = rs.random(m.shape) < 1 / 3
        img = np.where(near, np.where(m, ABOVE, np.where(rs.random(m.shape) < 0.5, HALF, BELOW)), img).astype(np.float32)
    return img


def fixed_nodes(m, ge=False):
    """the Dirichlet nodes of a mask image as include/diffnet_hip.h states them (dn_dirichlet): uint8 != 0, fp32 > 0.5.  ge: the wrong
    reading `>= 0.5` (test_comparator_has_teeth)"""
    if m is None:
        return None
    if m.dtype == np.uint8:
        return m != 0
    return (m >= HALF) if ge else (m > HALF)


# ---------------------------------------------------------------------------------------------
# the argument sets
# ---------------------------------------------------------------------------------------------
KINDS2 = [("f32", "u8"), ("u8", None), (None, "f32"), ("f32", "f32"), ("u8", "u8")]


def own_forms(family, P):
    if family == "strongform":
        return list(itertools.product((False, True), (False, True) if P > 1 else (False,)))         # NL, D2
    if family == "fosls":
        return [(False,), (True,)]                                                                    # NUF
    if family == "helmholtz":
        return [(0,), (1,), (2,)]                                                                     # CF
    return [()]


def part1_specs(family, P, ngp):
    """the full product of the host's selectors for one family, mode, degree and rule, as argument sets on the part-1 mesh"""
    fks = (0,) if family == "eikonal_vjp" else (0, 1, 2)
    forms = [(fk, m, *own) for fk in fks for m in (0, 1, 2) for own in own_forms(family, P)]
    base = 41 * DEGREE_RULES.index((P, ngp))         # 41: the rotations by i % 2 ... i % 5 differ between the (degree, rule) pairs
    return [Spec(family, P, ngp, *MESH1, PLAN1, f, base + i) for i, f in enumerate(forms)]


def widest(family, P, fk):
    own = dict(strongform=(True, P > 1), fosls=(True,), helmholtz=(2,)).get(family, ())
    return (fk, 2, *own)


def part2_specs(family):
    """every seam mesh at three (degree, rule) pairs with the widest form: Gauss-point forcing, and nodal forcing in a second case"""
    fks = (0,) if family == "eikonal_vjp" else (2, 1)
    return [Spec(family, P, ngp, nelx, nely, B, pl, widest(family, P, fk), 1000 + 10 * k + 2 * j + n)
            for k, (nelx, nely, B, pl) in enumerate(SEAMS) for j, (P, ngp) in enumerate(SEAM_RULES) for n, fk in enumerate(fks)]


def all_specs(family):
    return [s for P, ngp in DEGREE_RULES for s in part1_specs(family, P, ngp)] + part2_specs(family)


def _conditions(M, kinds, node_shape, B, i, key, seams, wide):
    """masks and values of the two conditions: M 0 none, 1 constants, 2 at least one value field; shared and per sample mixed by i.
    wide: both conditions, one fp32 and one uint8, a value field on each (part 2)"""
    masks, vals = [None, None], [0.0, 0.0]
    if M == 0:
        return masks, vals
    consts = (0.3125, -0.25)
    first_field = True
    for k in range(2):
        kind = kinds[k]
        if kind is None:
            continue
        masks[k] = mask_image(node_shape, B if (i + k) % 2 == 0 else 1, seams, kind, *key, k, thr=(i // 2) % 2 == 0)
        vals[k] = consts[k]
        if M == 2 and (wide or first_field or (i + k) % 3 == 0):
            vals[k] = rnd((B if (i + k) % 2 == 1 else 1, *node_shape), *key, "val", k)
            first_field = False
    return masks, vals


@functools.lru_cache(maxsize=None)
def build(spec):
    """the argument set of a spec: numpy float32 / uint8 arrays and Python floats, named as the operators' Python entries name them"""
    family, P, ngp, nelx, nely, B, pl, form, i = spec
    fk, M, own = form[0], form[1], form[2:]
    nx, ny = P * nelx + 1, P * nely + 1
    Bb = min(B, NREF)                                   # samples with inputs of their own
    key = tuple(spec)
    G = ngp * ngp
    shape = (ny, nx)
    wide = i >= 1000
    c = dict(spec=spec, family=family, P=P, ngp=ngp, B=B, nref=Bb, node_shape=shape, elem_shape=(nely, nelx), plan=pl)
    c["u"] = rnd((Bb, *shape), *key, "u", lo=-1.0, width=2.0)
    seams = seam_nodes(P, nx, ny, B, pl)
    kinds = ("f32", "u8") if wide else KINDS2[i % 5]
    c["masks"], c["vals"] = _conditions(M, kinds, shape, Bb, i, key, seams, wide)
    fB = Bb if (i // 2) % 2 == 0 else 1                 # the forcing: per sample or shared
    c["f"] = rnd((fB, *shape), *key, "f", lo=-2.0, width=4.0) if fk == 1 else None
    c["f_gp"] = rnd((fB, G, nely, nelx), *key, "fgp", lo=-2.0, width=4.0) if fk == 2 else (0.625 if i % 3 else (1.0 if family.startswith("eikonal") else 0.0))
    c["in_scale"] = IN_SCALE if (i % 2 and family in ("strongform", "fosls")) else None
    if family == "strongform":
        nl, d2 = own
        dxx, dyy = SF_C["d2"][i % 3] if d2 else (0.0, 0.0)
        c["coef"] = (SF_C["ax"], SF_C["ay"], SF_C["b"] if nl else 0.0, dxx, dyy, SF_C["fs"])
    elif family == "fosls":
        c["mx"], c["my"] = rnd((Bb, *shape), *key, "mx", lo=-2.0, width=4.0), rnd((Bb, *shape), *key, "my", lo=-0.25, width=0.5)
        c["nu"] = rnd((Bb if i % 2 == 0 else 1, *shape), *key, "nu", lo=0.5) if own[0] else (FO_C["nu"] if i % 3 else None)
    elif family == "helmholtz":
        cf = own[0]
        c["nu"], c["sigma"] = None, (HH_C["sigma"] if cf == 1 else 0.0)
        if cf == 2:
            which = ((True, True), (True, False), (False, True))[(i // 3) % 3] if not wide else (True, True)       # nu and sigma, nu only, sigma only
            if which[0]:
                c["nu"] = rnd((Bb if i % 2 == 0 else 1, *shape), *key, "nu", lo=0.5)
            c["sigma"] = rnd((Bb if i % 2 == 1 else 1, *shape), *key, "sigma", lo=-1.0, width=4.0) if which[1] else (HH_C["sigma"] if i % 2 else 0.0)
    elif family == "eikonal_vjp":
        c["cot"] = rnd((Bb, *shape), *key, "cot")
        c["in_num"], c["in_den"] = [(None, None), (IN_NUM, None), (IN_NUM, IN_DEN), (IN_NUM, 0.0)][2 if wide else i % 4]
        if i % 3 == 1:
            c["f"] = rnd((1, *shape), *key, "f")        # given and not read: dn_eikonal_apply passes no forcing on to the VJP
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
    """The kernel instantiation the host picks for an argument set, as (family and mode, P, NGP, MASK, BCF, FK, *own):
    elem2d_launch switches on degree * 10 + ngp; elem2d_launch_forms takes FK 2 for a Gauss-point forcing, else 1 for a nodal one, else
    0; elem2d_launch_mask takes MASK for any mask and BCF for a mask and any value field; SfFamily::launch adds NL (b != 0) and, above
    degree 1, D2 (dxx != 0 or dyy != 0); FoFamily::launch NUF (nu a field); HhFamily::launch CF (2: nu or sigma a field, 1: a constant
    sigma != 0, else 0); EkFamily::launch the VJP, for which dn_eikonal_apply has cleared both forcings (FK 0)."""
    fam, P, ngp = c["family"], c["P"], c["ngp"]
    assert (P, ngp) in DEGREE_RULES
    vjp = fam == "eikonal_vjp"
    fk = 0 if vjp else (2 if _is_field(c["f_gp"]) else (1 if c["f"] is not None else 0))
    mask = any(m is not None for m in c["masks"])
    bcf = mask and any(_is_field(v) for v in c["vals"])
    if fam == "strongform":
        ax, ay, b, dxx, dyy, fs = c["coef"]
        own = (b != 0.0, P > 1 and (dxx != 0.0 or dyy != 0.0))
    elif fam == "fosls":
        own = (_is_field(c["nu"]),)
    elif fam == "helmholtz":
        own = (2 if (c["nu"] is not None or _is_field(c["sigma"])) else (1 if c["sigma"] != 0.0 else 0),)
    else:
        own = ()
    return (fam, P, ngp, mask, bcf, fk, *own)


def expected_kernels(family):
    """the instantiations the dispatch can pick for one family and mode"""
    fks = (0,) if family == "eikonal_vjp" else (0, 1, 2)
    return {(family, P, ngp, mask, bcf, fk, *own) for P, ngp in DEGREE_RULES for fk in fks for mask, bcf in ((False, False), (True, False), (True, True))
            for own in own_forms(family, P)}


# ---------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables_f32(P, ngp):
    """the 1-D tables (N, dN, d2N, w) as dn_mesh and dn_strongform_args carry them: the reference's rule and basis, rounded to float32"""
    from diffnet_amd.tables import Basis1D, gauss_rule
    gx, gw = gauss_rule(ngp)
    return tuple(np.asarray(t, dtype=np.float32) for t in (*Basis1D(P).at_gauss(gx), gw))


def _lscale(c):
    """the scale of the VJP's cotangent (EkOp::start): in_num, / in_den where given, 0 at in_den == 0"""
    if c["in_num"] is None:
        return 1.0
    if c["in_den"] is None:
        return c["in_num"]
    return c["in_num"] / c["in_den"] if c["in_den"] > 0 else 0.0


def crop(c, ex, ey):
    """the case restricted to the elements [ex[0], ex[1]) x [ey[0], ey[1])"""
    P = c["P"]
    nod = lambda a: a[..., ey[0] * P:ey[1] * P + 1, ex[0] * P:ex[1] * P + 1] if _is_field(a) else a          # noqa: E731
    out = dict(c)
    for k in ("u", "mx", "my", "nu", "sigma", "cot", "f"):
        if k in out:
            out[k] = nod(out[k])
    out["masks"], out["vals"] = [nod(m) for m in c["masks"]], [nod(v) for v in c["vals"]]
    if _is_field(c["f_gp"]):
        out["f_gp"] = c["f_gp"][..., ey[0]:ey[1], ex[0]:ex[1]]
    out.update(node_shape=((ey[1] - ey[0]) * P + 1, (ex[1] - ex[0]) * P + 1), elem_shape=(ey[1] - ey[0], ex[1] - ex[0]))
    return out


def evaluate(c, single=False, scale=True, tables=None, ge=False, first_wins=False):
    """The restatement of the case's operator on the case's float32 values, per sample with inputs of its own.  Returns (outs, sums):
    outs a list with one entry per output field, dict(name, ref, S, fixed, exact) -- (nref, ny, nx) arrays: the values (float64, or
    float32 with `single`), the magnitude field, the nodes the operator zeroes and the exact 0 they hold; Helmholtz adds raw and S_raw,
    the field before out_scale, which its sumsq adds up -- and sums a dict name -> ((nref,) values, (nref,) magnitudes) of the sums the
    kernel adds up per element.  Deliberately wrong evaluations (test_comparator_has_teeth): tables (other 1-D tables), ge (`>= 0.5`),
    first_wins (condition 1 wins where both hold)."""
    from test_eikonal_host import eikonal_pullback_np, eikonal_t64
    from test_fosls_host import fosls_np
    from test_helmholtz_host import helmholtz_np
    from test_strongform_host import strongform_np
    fam, P, ngp, nref, shape = c["family"], c["P"], c["ngp"], c["nref"], c["node_shape"]
    npd, td = (np.float32, torch.float32) if single else (np.float64, torch.float64)
    tabs = tables_f32(P, ngp) if tables is None else tables
    names = NAMES[fam]
    acc = [collections.defaultdict(list, name=n) for n in names]
    sums = collections.defaultdict(lambda: ([], []))
    gs = OUT_SCALE * (1.0 if c["in_scale"] is None else c["in_scale"])            # exact: the kernel's out_scale * in_scale[0]
    for b in range(nref):
        masks = [fixed_nodes(pick(m, b), ge) if m is not None else None for m in c["masks"]]
        if first_wins and masks[0] is not None and masks[1] is not None:
            masks[1] = masks[1] & ~masks[0]
        vals = [pick(v, b) for v in c["vals"]]
        fx = np.zeros(shape, bool)
        for m in masks:
            if m is not None:
                fx |= m
        free = np.zeros(shape, bool)
        f = None if c["f"] is None else pick(c["f"], b)
        f_gp = pick(c["f_gp"], b)
        kw = dict(hx=HX, hy=HY, P=P, ngp=ngp, wscale=WSCALE, tables=tabs, masks=masks, vals=vals)
        if fam == "strongform":
            r = strongform_np(c["u"][b], coef=c["coef"], f=f, f_gp=f_gp, out_scale=gs, dtype=npd, scale=scale, **kw)
            res, mag, fixed = [r[1]], ([r[3][1]] if scale else None), [fx]
            sums["sum"][0].append(float(r[0])), sums["sum"][1].append(float(r[3][0]) if scale else 0.0)
        elif fam == "fosls":
            r = fosls_np(c["u"][b], c["mx"][b], c["my"][b], nu=1.0 if c["nu"] is None else pick(c["nu"], b), f=f, f_gp=f_gp,
                         weights=FO_C["weights"], fs=FO_C["fs"], out_scale=gs, dtype=npd, scale=scale, **kw)
            res, mag, fixed = list(r[1]), (list(r[3][1]) if scale else None), [fx, free, free]
            sums["sum"][0].append(float(r[0])), sums["sum"][1].append(float(r[3][0]) if scale else 0.0)
        elif fam == "helmholtz":
            r = helmholtz_np(c["u"][b], nu=None if c["nu"] is None else pick(c["nu"], b), sigma=pick(c["sigma"], b), f=f, f_gp=f_gp,
                             ecoef=HH_C["ecoef"], ocoef=HH_C["ocoef"], out_scale=OUT_SCALE, dtype=npd, scale=scale, **kw)
            res, mag, fixed = [r["out"]], ([r["S_out"]] if scale else None), [fx]
            acc[0]["raw"].append(r["raw"])
            acc[0]["S_raw"].append(r["S_raw"] if scale else np.zeros(shape, npd))
            sums["energy"][0].append(float(r["energy"])), sums["energy"][1].append(float(r["S_energy"]) if scale else 0.0)
        else:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)) if _is_field(a) else a       # noqa: E731
            ekw = dict(kw, masks=tuple(masks), **EK_C)
            if fam == "eikonal":
                ekw["vals"] = tuple(t(v) for v in vals)
                with torch.no_grad():
                    r = eikonal_t64(t(c["u"][b]), f=t(f_gp if f is None else f), dtype=td, scale=scale, **ekw)
                r = [x.numpy() for x in r] if scale else [r.numpy()]
            else:                                   # the scaled cotangent is exact (a power of two, or zero)
                ekw["vals"] = tuple(vals)
                r = eikonal_pullback_np(c["u"][b], c["cot"][b] * np.float32(_lscale(c)), dtype=npd, scale=scale, **ekw)
                r = list(r) if scale else [r]
            res, mag, fixed = [r[0]], ([r[1]] if scale else None), [fx]
        for k in range(len(names)):
            assert res[k].dtype == npd, (fam, res[k].dtype)
            acc[k]["ref"].append(res[k])
            acc[k]["S"].append(mag[k] if scale else np.zeros(shape, npd))
            acc[k]["fixed"].append(fixed[k])
            acc[k]["exact"].append(np.zeros(shape, np.float32))
    outs = [dict(name=a["name"], **{n: np.stack(v) for n, v in a.items() if n != "name"}) for a in acc]
    return outs, {n: (np.array(v), np.array(m)) for n, (v, m) in sums.items()}


@functools.lru_cache(maxsize=None)
def reference(spec):
    """float64 values, magnitude field, zeroed nodes and the element sums: computed once per session and left unchanged"""
    outs, sums = evaluate(build(spec))
    for o in outs:
        for a in o.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return outs, sums


# ---------------------------------------------------------------------------------------------
# the sums
# ---------------------------------------------------------------------------------------------
def n_roundings(family, P, ngp):
    """The float32 roundings on the longest path from the inputs to one element's sum (per element in fp32 over the G Gauss points, then
    fp64), counted from the kernels' formulas with NB = P + 1 fmas per 1-D stage; a product of two interpolated values carries both
    paths, a square twice its argument's:
      strong-form (sf_elem): a value or derivative 2 NB; the term b v u_x 4 NB + 1; r = fma(ax, ., fma(ay, ., fs f)) and the fmas of the
        NL and D2 terms 6 more: r 4 NB + 7; r^2 twice that; W r 1; esum = fma(Wr, r, esum) once per point: 2 (4 NB + 7) + 1 + G
      FOSLS (fo_elem): nu u_x 4 NB, q = fma(-nu, u_x, mx) 1: q 4 NB + 1; q^2 twice that; qy qy and fma(qx, qx, .) 2; Wq 1; two fmas into
        esum per point: 2 (4 NB + 1) + 3 + 2 G
      Helmholtz (hh_elem): Wk = W nu 2 NB + 1, c Wk 1, u_x^2 + u_y^2 4 NB + 2, their product 1: 6 NB + 5 (the reaction term 6 NB + 4, the
        forcing term 4 NB + 3); the two fmas that join the terms 2; esum += e once per point: 6 NB + 7 + G"""
    NB, G = P + 1, ngp * ngp
    return dict(strongform=2 * (4 * NB + 7) + 1 + G, fosls=2 * (4 * NB + 1) + 3 + 2 * G, helmholtz=6 * NB + 7 + G)[family]


def element_sum_bound(spec, vals, mags, weight):
    """(the float64 sum, its bound n 2^-24 (the same sum over the magnitudes)); weight: how often each sample counts"""
    w = np.asarray(weight, dtype=np.float64)
    return float((w * vals).sum()), n_roundings(spec.family, spec.P, spec.ngp) * U * float((w * mags).sum())


@functools.lru_cache(maxsize=None)
def yardstick(family):
    """Y: the largest e of the float32 CPU evaluation of the restatement over every case of the family and mode; (Y, the case)"""
    worst, where = 0.0, None
    for spec in all_specs(family):
        ref, _ = reference(spec)
        single, _ = evaluate(build(spec), single=True, scale=False)
        for o, s in zip(ref, single):
            assert s["ref"].dtype == np.float32
            e, at = node_error(s["ref"], o, strict=False)
            assert math.isfinite(e), (spec, o["name"], at)
            if e > worst:
                worst, where = e, (spec, o["name"], at)
    return worst, where
