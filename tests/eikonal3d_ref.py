"""What test_gpu_eikonal3d_forms.py needs and no GPU: the argument sets of dn_eikonal3d_apply as plain numpy data, a Python mirror of the
launch plan (ek3_plan in csrc/eikonal3d.hip: the default rule and the "PLAN3D" override with its acceptance conditions) and of the kernel
selection (ek3_launch_forms, ek3_launch_mask), the float64 restatement of the operator and of its VJP with the magnitude field, the
comparator, the yardstick and the bound of the sums.

The restatement is the formula in the header of dn_eikonal3d_apply (include/diffnet_hip.h), per sample:
    u~ = u after condition 1 then condition 2;  at a Gauss point  A = sq |grad u~|^2 - f,  (B, C, D) = tau u~ grad u~
    R_a = zero_on_dirichlet(sum_e sum_g W_g (N_a A + Nx_a B + Ny_a C + Nz_a D)),   W_g = w_g wscale
    VJP: cot' = cot in_num / in_den, zero on the Dirichlet nodes, evaluated like a field (L, grad L):
         A' = tau grad L . grad u~,  (B', C', D') = 2 sq L grad u~ + tau u~ grad L  in the same flux form
evaluated in float64 (the reference) and in float32 (the yardstick) by the same code on the float32 values the kernel reads: fields, masks,
forcing, cotangent, the constants (short dyadic numbers; the spacings are powers of two and differ per axis, so every 2 / h is exact) and
the 1-D tables as dn_mesh stores them (float32).  The magnitude field S is the same formula with every input, table entry and constant
replaced by its absolute value and the subtraction of f made an addition, after the Dirichlet substitutions, 0 where the operator writes 0
(as elem2d_ref.py does).  A result is judged node by node: e = |got - ref64| / S on the free nodes (S == 0: exactly 0), exactly 0 on the
Dirichlet nodes.  The bound is K = MARGIN * Y, Y (the yardstick) being the largest e the float32 evaluation of the same restatement reaches
over all the cases of the file with the same mode (R, VJP): it is measured against the reference alone."""
import collections
import functools
import itertools
import math
import zlib

import numpy as np

from poisson3d_ref import HS
from q1_residual_ref import MARGIN, U

TAU, SQ, WSCALE, FCONST = 0.25, 1.375, 0.25, 0.75          # sq != 1 + tau, wscale != 1; tau is 0 in one case of five
VALS = (0.3125, -0.25)                                     # the two conditions' constants
MESH1, PLAN1 = (17, 9, 7), "8,8,1,3"                       # part 1 (elements): 3 chunks x 2 tiles x 3 strips x B = 2 one-wave workgroups
RULES = (2, 3, 4)
CONDS = ("none", "const", "field")
FORMS = [(cond, fk, False) for cond in CONDS for fk in (0, 1, 2)] + [(cond, 0, True) for cond in CONDS]      # 12 per rule
KINDS = [("f32", "u8"), ("u8", "bool"), ("bool", "f32"), ("f32", "f32"), ("u8", "u8")]
PRESENT = ("both", "first", "both", "second", "both", "both")

Case = collections.namedtuple("Case", "name ngp cond fk vjp nel B plan i")
# cond: "none" | "const" | "field" (MASK, BCF); fk: 0 constant, 1 nodal, 2 Gauss-point forcing; nel: (nelx, nely, nelz); plan: "PLAN3D"
# ("" the default); i: what varies inside a form -- mask formats, shared / per-sample arrays, which conditions exist, tau, in_num / in_den


# ---------------------------------------------------------------------------------------------
# the launch plan (ek3_plan) and the kernel selection (ek3_launch_forms, ek3_launch_mask), mirrored
# ---------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def tiles_for(n, T):
    """tiles of T threads that overlap by one thread cover n node columns (or rows)"""
    return 1 if n <= T else _cdiv(n - 1, T - 1)


def plan_accepted(plan):
    """the override's acceptance conditions: four integers, TX, TY >= 2, TX * TY <= 256 and a multiple of 64, R >= 1"""
    try:
        TX, TY, _, R = (int(x) for x in plan.split(","))
    except ValueError:
        return False
    return TX >= 2 and TY >= 2 and TX * TY <= 256 and (TX * TY) % 64 == 0 and R >= 1


def geometry(nodes, B, plan=""):
    """ek3_plan for a mesh of `nodes` = (nx, ny, nz) and the "PLAN3D" value in force: TX, TY, R, chunks, tiles, strips, and what the kernel
    makes of them: grid (workgroups), waves per workgroup, per strip the layers it marches (the recomputed one under its first node plane
    plus its own) and its own layers"""
    nx, ny, nz = nodes
    nelz = nz - 1
    TX, TY, best = 16, 16, -1.0
    for ty in (4, 8, 12, 16):
        util = ny / (tiles_for(ny, ty) * ty) + 0.002 * ty
        if util > best:
            best, TY = util, ty
    R = 32
    per_strip = tiles_for(nx, TX) * tiles_for(ny, TY) * B
    while R > 4 and per_strip * _cdiv(nelz, R) < 1024:
        R //= 2
    if plan and plan_accepted(plan):
        TX, TY, _, R = (int(x) for x in plan.split(","))
    R = max(1, min(R, nelz))
    g = dict(TX=TX, TY=TY, R=R, chunks=tiles_for(nx, TX), tiles=tiles_for(ny, TY), strips=_cdiv(nelz, R))
    g["grid"] = g["chunks"] * g["tiles"] * g["strips"] * B
    g["waves"] = TX * TY // 64
    g["own"] = [min(s * R + R, nelz) - s * R for s in range(g["strips"])]
    g["layers"] = [n + (1 if s > 0 else 0) for s, n in enumerate(g["own"])]
    return g


def column_owners(nodes, g):
    """per chunk: [(node column, whether the owning thread has an element)] -- `owner` and `elem_ok` of the kernel along x"""
    nx = nodes[0]
    out = []
    for chunk in range(g["chunks"]):
        cols = [chunk * (g["TX"] - 1) + tx for tx in range(g["TX"]) if not (chunk > 0 and tx == 0)]
        out.append([(x, x < nx - 1) for x in cols if x < nx])
    return out


def seam_lines(nodes, g):
    """(columns, rows, planes): the node lines on both sides of every chunk, tile and strip seam of a geometry, plus the last of each"""
    nx, ny, nz = nodes
    cols = {k * (g["TX"] - 1) + d for k in range(1, g["chunks"]) for d in (-1, 0, 1)} | {nx - 1}
    rows = {k * (g["TY"] - 1) + d for k in range(1, g["tiles"]) for d in (-1, 0, 1)} | {ny - 1}
    planes = {k * g["R"] + d for k in range(1, g["strips"]) for d in (-1, 0, 1)} | {nz - 1}
    return tuple(sorted(x for x in s if 0 <= x < n) for s, n in ((cols, nx), (rows, ny), (planes, nz)))


def dispatch(c):
    """the template arguments the host picks for an argument set: (NGP, MASK, BCF, FK, VJP)"""
    conds = [m for m in c["conds"] if m is not None]
    vjp = c["cot"] is not None
    fk = 0 if vjp else {None: 0, "nodal": 1, "gp": 2}[c["fkind"]]
    return (c["ngp"], bool(conds), any(isinstance(m["value"], np.ndarray) for m in conds), fk, vjp)


def is_pf(sel):
    """PF of eikonal3d_kernel: the next plane's loads stay in flight across a layer"""
    _, mask, _, fk, vjp = sel
    return not vjp and not (mask and fk != 0)


# ---------------------------------------------------------------------------------------------
# seeded data
# ---------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def rnd(shape, *key, lo=-0.5, width=1.0):
    return (lo + width * _rng(*key).random(shape)).astype(np.float32)


def pick(a, b):
    return a[b if a.shape[0] > 1 else 0]


def distance_field(nodes, B, *key):
    """The field of tests/test_gpu_eikonal3d.py -- the distance to the centre of the box (|grad u| = 1) plus h x noise in (-1/2, 1/2), h the
    spacing along x -- with the constant 0.25 in place of -0.3, so that u exceeds 0.5 on a part of every mesh, the one-element mesh included
    (what an absent mask must not be mistaken for: the kernel's dummy mask read is the load of u)"""
    ax = [np.arange(n) * h - 0.5 * (n - 1) * h for n, h in zip(nodes, HS)]
    r = np.sqrt(ax[0][None, None, :] ** 2 + ax[1][None, :, None] ** 2 + ax[2][:, None, None] ** 2) + 0.25
    nx, ny, nz = nodes
    return (r[None] + HS[0] * (_rng("u", *key).random((B, nz, ny, nx)) - 0.5)).astype(np.float32)


HALF = np.float32(0.5)
EDGE = np.array([HALF, np.nextafter(HALF, np.float32(0)), np.nextafter(HALF, np.float32(1))], dtype=np.float32)     # free, free, fixed


def mask_image(nodes, Bm, kind, lines, off, *key):
    """(Bm, nz, ny, nx): a 10 % blob per sample (none on meshes below 64 nodes); on every seam line (and the last column, row and plane) one node of four fixed and two of
    four free along the other axes, in the same phase for both conditions (they overlap there); condition 1 holds the first corner, condition
    2 the first and the last.  "u8": 0 / 1 / 2 / 255; "bool"; "f32": 0 / 1, and on meshes of 64 nodes or more 8 % of the nodes take exactly
    0.5 or one of its two float32 neighbours (0.5 and the one below are free: `> 0.5`)."""
    nx, ny, nz = nodes
    rs = _rng("mask", *key)
    m = rs.random((Bm, nz, ny, nx)) < (0.10 if nx * ny * nz >= 64 else 0.0)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ph = (x + y + z + off) % 4
    cols, rows, planes = lines
    on = np.isin(x, cols) | np.isin(y, rows) | np.isin(z, planes)
    m[:, on & (ph == 0)] = True
    m[:, on & ((ph == 1) | (ph == 2))] = False
    m[:, 0, 0, 0] = True
    if key[-1] == 1:
        m[:, nz - 1, ny - 1, nx - 1] = True
    if kind == "bool":
        return m
    if kind == "u8":
        return np.where(m, np.array([1, 2, 255], np.uint8)[rs.integers(0, 3, m.shape)], 0).astype(np.uint8)
    img = m.astype(np.float32)
    if nx * ny * nz < 64:
        return img
    edge = rs.random(m.shape) < 0.08
    edge[:, 0, 0, 0] = False
    return np.where(edge, EDGE[rs.integers(0, 3, m.shape)], img).astype(np.float32)


def fixed_nodes(img, ge=False):
    """the Dirichlet nodes of a mask image: uint8 / bool != 0, fp32 > 0.5 (dn_dirichlet).  ge: the wrong `>=`"""
    if img.dtype == np.float32:
        return (img >= HALF) if ge else (img > HALF)
    return img != 0


@functools.lru_cache(maxsize=None)
def tables(ngp):
    """(N, dN, w) as dn_mesh carries them (FemGeometry.mesh_struct): float32"""
    from diffnet_amd.tables import Basis1D, gauss_rule
    gx, gw = gauss_rule(ngp)
    Bv, Dv, _ = Basis1D(1).at_gauss(gx)
    return tuple(np.asarray(t, dtype=np.float32) for t in (Bv, Dv, gw))


# ---------------------------------------------------------------------------------------------
# the argument sets
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build(case):
    """the argument set of a case: numpy float32 / uint8 / bool arrays (fields without the channel axis) and Python floats.
    conds: two entries, None or dict(img, value); fkind: None (the constant f) | "nodal" | "gp"; cot: None or the cotangent (the VJP)"""
    name, ngp, cond, fk, vjp, nel, B, plan, i = case
    nodes = tuple(n + 1 for n in nel)
    nx, ny, nz = nodes
    shape = (nz, ny, nx)
    key = tuple(case)
    c = dict(case=case, ngp=ngp, nodes=nodes, nel=nel, B=B, plan=plan, shape=shape, tables=tables(ngp), tau=0.0 if i % 5 == 4 else TAU, sq=SQ,
             wscale=WSCALE, fconst=FCONST)
    c["u"] = distance_field(nodes, B, *key)
    # the forcing (the VJP reads none)
    fb = B if (i // 2) % 2 == 0 else 1
    c["fkind"], c["f"] = None, None
    if fk == 1 and not vjp:
        c["fkind"], c["f"] = "nodal", rnd((fb, *shape), *key, "f", lo=0.5)
    elif fk == 2 and not vjp:
        c["fkind"], c["f"] = "gp", rnd((fb, ngp ** 3, nz - 1, ny - 1, nx - 1), *key, "fgp", lo=0.5)
    # the conditions: their masks carry the seam pattern of the case's plan AND of the default plan (every case runs under both)
    c["conds"] = [None, None]
    if cond != "none":
        present = name[4:] if name.startswith("only") else ("both" if name == "threshold" else PRESENT[i % 6])
        here = dict(both=(0, 1), first=(0,), second=(1,))[present]
        lines = [sorted(set(a) | set(b)) for a, b in zip(seam_lines(nodes, geometry(nodes, B, plan)), seam_lines(nodes, geometry(nodes, B)))]
        off = 0 if nx * ny * nz < 64 else int(_rng("offset", *key).integers(0, 4))
        kinds = KINDS[i % 5]
        fields = [(True, False), (False, True), (True, True)][i % 3] if cond == "field" else (False, False)
        if cond == "field" and not any(fields[k] for k in here):
            fields = (True, True)
        for k in here:
            img = mask_image(nodes, B if (i + k) % 2 == 0 else 1, kinds[k], lines, off, *key, k)
            value = rnd((B if (i + k) % 2 == 1 else 1, *shape), *key, "val", k, lo=0.25, width=0.5) if fields[k] else VALS[k]
            c["conds"][k] = dict(img=img, value=value)
        if name == "threshold":               # condition 1: nothing but the three nodes; condition 2 leaves them alone
            img = np.zeros((1, *shape), np.float32)
            for v, at in zip(EDGE, EDGE_NODES):
                img[(0, *at)] = v
                c["conds"][1]["img"][(slice(None), *at)] = 0
            c["conds"][0]["img"] = img
    # the VJP: a cotangent that is not zero on the Dirichlet nodes; no in_num, in_num alone, in_num with in_den
    c["cot"], c["in_num"], c["in_den"] = None, None, None
    if vjp:
        c["cot"] = rnd((B, *shape), *key, "cot")
        c["in_num"], c["in_den"] = [(None, None), (1.5, None), (1.5, 0.75)][i % 3]
    return c


def part1_cases():
    """the full product: 3 rules x 12 forms on MESH1 with B = 2 under PLAN1"""
    return [Case("part1", ngp, cond, fk, vjp, MESH1, 2, PLAN1, 12 * r + k) for r, ngp in enumerate(RULES) for k, (cond, fk, vjp) in enumerate(FORMS)]


# part 2: (elements, B, plan).  What each reaches is asserted by test_seam_list_reaches_every_property
SEAMS = [((1, 1, 1), 1, ""), ((15, 3, 2), 1, ""), ((16, 3, 1), 2, ""), ((17, 16, 3), 1, ""), ((17, 5, 3), 2, "16,4,1,1"), ((9, 5, 7), 1, "16,4,1,2"),
         ((9, 5, 7), 2, "16,4,1,3"), ((9, 7, 5), 1, "8,8,1,2"), ((40, 3, 4), 1, "32,2,1,3"), ((20, 17, 5), 1, "16,16,1,4"), ((130, 3, 6), 1, "128,2,1,5"),
         ((70, 3, 5), 2, "64,2,1,2"), ((5, 40, 9), 1, "2,32,1,4"), ((17, 16, 5), 2, "")]
# one PF forward kernel, one non-PF forward kernel and one VJP kernel per rule: (cond, fk, vjp)
SEAM_FORMS = [("const", 0, False), ("field", 2, False), ("field", 0, True)]


def part2_cases():
    out = []
    for k, (nel, B, plan) in enumerate(SEAMS):
        for r, ngp in enumerate(RULES):
            for n, (cond, fk, vjp) in enumerate(SEAM_FORMS):
                out.append(Case("seam", ngp, cond, fk, vjp, nel, B, plan, 100 + 9 * k + 3 * r + n))
    return out


BATCH_NEL, BATCH_B, BATCH_BASE = (2, 2, 2), 600, 3


def batch_cases():
    """the large batch: the three distinct samples the B = 600 launch cycles through (the reference is computed for these only)"""
    return [Case("batch", ngp, cond, fk, vjp, BATCH_NEL, BATCH_BASE, "", 300 + 3 * r + n)
            for r, ngp in enumerate(RULES) for n, (cond, fk, vjp) in enumerate(SEAM_FORMS)]


def only_cases():
    """exactly one condition: condition 1 alone and condition 2 alone, in every mask format, constants and value fields, forward (both
    schedules) and VJP.  u exceeds 0.5 on free nodes: a kernel that took its dummy read of u for the absent mask is seen"""
    out = []
    for n, (which, (cond, fk, vjp)) in enumerate(itertools.product(("first", "second"), SEAM_FORMS)):
        for d in range(3):
            out.append(Case("only" + which, RULES[(n + d) % 3], cond, fk, vjp, (9, 6, 5), 2, "8,8,1,2", 400 + 5 * n + d))
    return out


EDGE_NEL = (9, 6, 5)
EDGE_NODES = [(2, 3, 4), (3, 2, 7), (4, 4, 2)]            # (z, y, x) of the nodes at 0.5, its lower and its upper neighbour


def threshold_cases():
    """fp32 masks that are zero but for three interior nodes at 0.5 and its two neighbours, on one form per schedule"""
    return [Case("threshold", RULES[n], cond, fk, vjp, EDGE_NEL, 1, "8,8,1,2", 500 + n) for n, (cond, fk, vjp) in enumerate(SEAM_FORMS)]


def all_cases():
    return part1_cases() + part2_cases() + batch_cases() + only_cases() + threshold_cases()


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
_CORNERS = list(itertools.product((0, 1), repeat=3))                   # (kz, ky, kx)


def eikonal3d(u, fixed, vals, f, fkind, cot, lscale, tabs, tau, sq, wscale, *, dtype=np.float64, hs=HS, magnitude=False, mutate=None):
    """dn_eikonal3d_apply on one sample (nz, ny, nx) or on a batch of them (any leading axes).  fixed / vals: the conditions in order (boolean
    images; constants or nodal fields); f: a float, a nodal field or (fkind "gp") (..., G, nelz, nely, nelx), x fastest in G; cot: None (R) or
    the cotangent (the VJP; lscale: in_num / in_den).  Every operation is done in `dtype`.  magnitude: the field S of the module docstring.
    mutate: a deliberately wrong evaluation (test_comparator_has_teeth).  Returns (out, the union of the Dirichlet nodes)."""
    dt = dtype
    ab = np.abs if magnitude else (lambda a: a)
    N, dN, w = (ab(np.asarray(t, dtype=np.float64).astype(dt)) for t in tabs)
    ngp = len(w)
    sc = [dt(2.0) / dt(h) for h in hs]
    tau, sq, wscale = (ab(dt(np.float32(x))) for x in (tau, sq, wscale))
    sq2 = sq if mutate == "sq2" else dt(2.0) * sq
    ut = u.astype(dt)
    fx = np.zeros(u.shape, bool)
    for m, v in zip(fixed, vals):
        ut = np.where(m, np.asarray(v, dtype=np.float32).astype(dt), ut)
        fx = fx | m
    ut = ab(ut)
    nz, ny, nx = u.shape[-3:]
    sl = {k: np.s_[..., k[0]:nz - 1 + k[0], k[1]:ny - 1 + k[1], k[2]:nx - 1 + k[2]] for k in _CORNERS}
    Uc = {k: np.ascontiguousarray(ut[sl[k]]) for k in _CORNERS}
    vjp = cot is not None
    if vjp:
        lt = cot.astype(dt) * dt(lscale)
        lt = ab(lt if mutate == "cot" else np.where(fx, dt(0), lt))
        Lc = {k: np.ascontiguousarray(lt[sl[k]]) for k in _CORNERS}
    elif fkind == "nodal":
        Fc = {k: np.ascontiguousarray(ab(f.astype(dt))[sl[k]]) for k in _CORNERS}
    out = np.zeros(u.shape, dt)
    for gz, gy, gx in itertools.product(range(ngp), repeat=3):
        W = w[gx] * w[gy] * w[gz] * wscale
        Nc = {k: N[gx, k[2]] * N[gy, k[1]] * N[gz, k[0]] for k in _CORNERS}
        Dx = {k: dN[gx, k[2]] * sc[0] * N[gy, k[1]] * N[gz, k[0]] for k in _CORNERS}
        Dy = {k: N[gx, k[2]] * dN[gy, k[1]] * sc[1] * N[gz, k[0]] for k in _CORNERS}
        Dz = {k: N[gx, k[2]] * N[gy, k[1]] * dN[gz, k[0]] * sc[2] for k in _CORNERS}
        at = lambda C, T: sum(T[k] * C[k] for k in _CORNERS)                    # noqa: E731
        ug, ux, uy, uz = at(Uc, Nc), at(Uc, Dx), at(Uc, Dy), at(Uc, Dz)
        if mutate == "dz" and gz == 1:
            uz = uz * dt(0)
        if vjp:
            L, Lx, Ly, Lz = at(Lc, Nc), at(Lc, Dx), at(Lc, Dy), at(Lc, Dz)
            A = tau * (Lx * ux + Ly * uy + Lz * uz)
            Bc, Cc, Dc = sq2 * L * ux + tau * ug * Lx, sq2 * L * uy + tau * ug * Ly, sq2 * L * uz + tau * ug * Lz
        else:
            if fkind == "nodal":
                fg = at(Fc, Nc)
            elif fkind == "gp":
                g = (gx * ngp + gy) * ngp + gz if mutate == "gp_order" else (gz * ngp + gy) * ngp + gx
                fg = ab(f[..., g, :, :, :].astype(dt))
            else:
                fg = ab(dt(np.float32(f)))
            A = sq * (ux * ux + uy * uy + uz * uz) + (fg if magnitude else -fg)
            Bc, Cc, Dc = tau * ug * ux, tau * ug * uy, tau * ug * uz
        for k in _CORNERS:
            out[sl[k]] += W * (Nc[k] * A + Dx[k] * Bc + Dy[k] * Cc + Dz[k] * Dc)
    out = np.where(fx, dt(0), out)
    assert out.dtype == dt
    return out, fx


def _mutant_tables(tabs):
    """the 4-point rule with the first 1-D weight replaced by its neighbour"""
    N, dN, w = tabs
    assert len(w) == 4 and w[0] != w[1]
    w = w.copy()
    w[0] = w[1]
    return N, dN, w


def evaluate(c, *, dtype=np.float64, magnitude=False, mutate=None):
    """The restatement on every sample of an argument set: (out, fixed), both (B, nz, ny, nx)"""
    B = c["B"]
    full = lambda a: np.broadcast_to(a, (B, *a.shape[1:]))                     # noqa: E731
    conds = [m for m in c["conds"] if m is not None]
    fixed = [full(fixed_nodes(m["img"], ge=mutate == "ge")) for m in conds]
    vals = [full(m["value"]) if isinstance(m["value"], np.ndarray) else m["value"] for m in conds]
    if mutate == "order":
        fixed, vals = fixed[::-1], vals[::-1]
    f = c["fconst"] if c["fkind"] is None else full(c["f"])
    lscale = 1.0
    if c["cot"] is not None and c["in_num"] is not None:
        lscale = dtype(np.float32(c["in_num"])) / (dtype(np.float32(c["in_den"])) if c["in_den"] is not None else dtype(1))
    tabs = _mutant_tables(c["tables"]) if mutate == "weight" else c["tables"]
    return eikonal3d(c["u"], fixed, vals, f, c["fkind"], c["cot"], lscale, tabs, c["tau"], c["sq"], c["wscale"], dtype=dtype, magnitude=magnitude,
                     mutate=mutate)


def seam_layer_left_out(c, ref, z0, b=0):
    """ref["out"] with the layer under node plane z0 missing from that plane on sample b: what a strip that starts at z0 and does not
    recompute the layer below would write"""
    one = dict(c, B=1, u=c["u"][b:b + 1, z0 - 1:z0 + 1], cot=None if c["cot"] is None else c["cot"][b:b + 1, z0 - 1:z0 + 1])
    one["conds"] = [None if m is None else dict(img=pick(m["img"], b)[None, z0 - 1:z0 + 1],
                                                 value=pick(m["value"], b)[None, z0 - 1:z0 + 1] if isinstance(m["value"], np.ndarray) else m["value"])
                    for m in c["conds"]]
    if c["fkind"] == "nodal":
        one["f"] = pick(c["f"], b)[None, z0 - 1:z0 + 1]
    elif c["fkind"] == "gp":
        one["f"] = pick(c["f"], b)[None, :, z0 - 1:z0]
    share = evaluate(one)[0][0, 1]
    out = ref["out"].copy()
    out[b, z0] -= share
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """float64 values, magnitudes and sums of a case: computed once per session and left unchanged"""
    c = build(case)
    out, fx = evaluate(c)
    S = evaluate(c, magnitude=True)[0]
    r = dict(out=out, S=S, fixed=fx, sumsq=float((out * out).sum()), abs_S=float((np.abs(out) * S).sum()), S2=float((S * S).sum()), n=out.size)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


# ---------------------------------------------------------------------------------------------
# the comparator and the bounds
# ---------------------------------------------------------------------------------------------
def node_error(got, ref):
    """e = |got - ref64| / S per node; inf where a rule is broken: a non-finite value, a free node without a term that is not exactly 0, a
    Dirichlet node that is not exactly 0.  Returns (max e, its index)."""
    got = np.asarray(got).astype(np.float64)
    r, S, fixed = ref["out"], ref["S"], ref["fixed"]
    assert got.shape == r.shape, (got.shape, r.shape)
    pos = S > 0
    e = np.where(pos, np.abs(got - r) / np.where(pos, S, 1.0), np.where(got == 0.0, 0.0, math.inf))
    e = np.where(fixed, np.where(got == 0.0, 0.0, math.inf), e)
    e = np.where(np.isfinite(got), e, math.inf)
    at = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[at]), tuple(int(x) for x in at)


def mode(case):
    return "VJP" if case.vjp else "R"


@functools.lru_cache(maxsize=None)
def yardsticks():
    """Y per mode: (the largest e of the float32 evaluation of the restatement over every case of the file, the case)"""
    Y = {}
    for case in all_cases():
        e, at = node_error(evaluate(build(case), dtype=np.float32)[0], reference(case))
        assert math.isfinite(e), (case, at)
        if e > Y.get(mode(case), (0.0, None))[0]:
            Y[mode(case)] = (e, case)
    return Y


def K_of(case):
    return MARGIN * yardsticks()[mode(case)][0]


def sumsq_bound(ref, K, times=1):
    """The bound of |sumsq - sum ref64^2| (`times`: the reference's samples occur that often in the launch).
    emit_plane adds (double)(t * t) per owned node, t the float32 value the node gets: the square is ONE float32 multiplication,
    fl(t^2) = t^2 (1 + d) with |d| <= 2^-24 (a product below the normal range: within 2^-149 of t^2); every addition after it -- per thread,
    block_sum, the last arriver's fixed-order sum of dn_reduce.h -- is a float64 addition of non-negative numbers, n of them at most for n
    nodes: a relative n 2^-53 of the total.  With t = r + d_a, |d_a| <= K S_a on the free nodes (the node bound) and t = r = 0 on the others,
        |t^2 - r^2| <= 2 K |r| S_a + K^2 S_a^2,  so  sum t^2 <= T := sum r^2 + 2 K sum |r| S + K^2 sum S^2  and
        |sumsq - sum r^2| <= 2 K sum |r| S + K^2 sum S^2 + (2^-24 + n 2^-53) T + n 2^-149.
    The rounding term is 2^-24 (one multiplication) times T; no second float32 rounding exists between a node's value and the sum."""
    n = ref["n"] * times
    first = times * (2.0 * K * ref["abs_S"] + K * K * ref["S2"])
    T = times * ref["sumsq"] + first
    return first + (U + n * 2.0 ** -53) * T + n * 2.0 ** -149


def norm_interval(ref, K, times=1):
    """norm = (float)sqrt(sumsq): the interval of sumsq taken through the square root (correctly rounded in float64: 2^-53 relative) and one
    float32 rounding of the stored value (2^-24 relative)"""
    s, b = times * ref["sumsq"], sumsq_bound(ref, K, times)
    r = U + 2.0 ** -52
    return math.sqrt(max(s - b, 0.0)) * (1.0 - r), math.sqrt(s + b) * (1.0 + r)
