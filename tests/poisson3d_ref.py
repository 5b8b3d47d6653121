"""What test_gpu_poisson3d_forms.py needs and no GPU: the argument sets of dn_poisson_apply on 3-D Q1 meshes as plain numpy data, a Python
mirror of the host's choice (poisson_choose, plan3d, plan3d_env in csrc/poisson_fused.hip; launch3_flags, launch3_one, launch3_f32n,
launch3_n2, launch3_n2_bc in csrc/poisson3d_q1.inl; launch_cf3_bc in csrc/poisson3d_q1_cf.hip), the float64 restatement of the operator with
its per-node scale, the comparator and the yardstick.

The restatement is the formula in the header of dn_poisson_args (include/diffnet_hip.h), per sample:
    out_a = out_scale * zero_on_dirichlet(sum_e sum_g W_g (alpha nu_g gradN_a . grad u~_g - beta N_a f_g)),   W_g = w_g wscale
    E1 = sum W nu |grad u~|^2,  E2 = sum W u~ f,  energy = c E1 - E2,  sumsq = sum (out / out_scale)^2
(load vector b: out_a -= beta wscale b_a, E2 = wscale sum_a u~_a b_a), evaluated in float64 on the float32 values the kernel reads: fields,
masks, forcing, constants (all exactly representable: the spacings are powers of two, so every scale[d] is one) and the 1-D tables as
dn_mesh stores them (float32).  With `scale=True` it also returns S_a, the sum of |W_g t| over the placed terms that make up node a's value
(one term per element and Gauss point: t = alpha nu_g gradN_a . grad u~_g - beta N_a f_g; the load vector's share is one more term), SE1 / SE2,
the same sums for the two energy integrals, and SN = sum_a |u~_a| S_a.  A result is judged node by node: e = |got - ref64| / (|out_scale| S_a) on the free nodes
(S_a == 0: exactly 0), exactly 0 on the Dirichlet nodes.  The bound is K = MARGIN * Y, Y (the yardstick) being the largest e the float32
evaluation of the same restatement reaches over all the cases of this file with the same rule and forcing form."""
import collections
import functools
import itertools
import math
import zlib

import numpy as np

from q1_residual_ref import MARGIN, U

HS = (0.125, 0.25, 0.5)                       # hx, hy, hz: scale[d] = 2 / h = 16, 8, 4
CONST = dict(alpha=1.5, beta=0.75, c=0.75, wscale=0.25, out_scale=0.5, energy_scale=0.125)
A2 = 0.5773502691896258
RULES = {"g2": ([-A2, A2], [1.0, 1.0]),            # the exact 2-point rule
         "u2": ([-0.5, 0.7], [1.0, 1.0]),          # unit weights, unsymmetric points: basis[0][1] + basis[1][1] != 1 (poisson_choose: no closed form in z)
         "w2": ([-A2, A2], [0.5, 1.5]),            # non-unit weights: the one-element forms with UW = false
         "g3": None, "g4": None}                   # the reference's (truncated) literals: diffnet_amd.tables.gauss_rule
NGP = dict(g2=2, u2=2, w2=2, g3=3, g4=4)
FACES = dict(xlo=1, xhi=2, ylo=4, yhi=8, zlo=16, zhi=32)
FAM = {4: "n1", 5: "t16", 6: "generic", 7: "n2", 8: "cfz"}            # DN_POISSON_3D_Q1_*
FAMILIES = ("cfz", "n2", "n1", "t16", "generic")
MESH_E, MESH_O = (34, 17, 6), (33, 17, 6)          # part 1: two chunks, two tiles, two strips (R = 3 of 5 layers: a shorter last strip)
PLAN1 = dict(cfz="16,16,2,3", n2="16,16,2,3", n1="16,16,1,3", t16="16,8,1,3", generic="32,8,1,3")

Case = collections.namedtuple("Case", "family rule base cond mesh B plan route i")
# base: a string of the letters N (nu), F (nodal f), G (f at Gauss points), L (f is the load vector); cond: see _cond_list
# route: what keeps E1G off ("sums": nothing, sums wanted; "nosums"; "alpha0"; "e1sum") and, N2, what sends the launch there ("n2", "u2")


# ---------------------------------------------------------------------------------------------
# the launch plan (plan3d, plan3d_env) and the host's choice (poisson_choose), mirrored
# ---------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def chunks_for(n, T):
    return 1 if n <= T else _cdiv(n - 1, T - 1)


def _strip_height(wg_per_strip, nelz, cap):
    best, R = 1e300, max(nelz, 1)
    for r in range(4, min(64, max(nelz, 4)) + 1):
        strips = _cdiv(nelz, r)
        rounds = max(1.0, math.ceil(2.0 * (wg_per_strip * strips) / cap) / 2.0)
        layers = (nelz if strips == 1 else r + 1) + 1.5
        cost = rounds * layers * (1.0 + 0.002 * r)
        if cost < best:
            best, R = cost, r
    return max(nelz, 1) if R > nelz else R


def plan3d(ngp, mesh, B, allow_e2):
    nx, ny, nz = mesh
    nelz = nz - 1
    if ngp == 2 and allow_e2:
        g = dict(TX=16, TY=16, E=2, chunks=chunks_for(nx // 2, 16), tiles=chunks_for(ny, 16))
        g["R"] = _strip_height(g["chunks"] * g["tiles"] * B, nelz, 256.0 * 3.0)
    elif ngp == 2:
        g = dict(TX=16, E=1, chunks=chunks_for(nx, 16))
        best = -1.0
        for TY in (4, 8, 12, 16):
            tiles = chunks_for(ny, TY)
            util = ny / (tiles * TY) + 0.002 * TY
            if util > best:
                best, g["TY"], g["tiles"] = util, TY, tiles
        g["R"] = _strip_height(g["chunks"] * g["tiles"] * B, nelz, 256.0 * 5.0 * (256.0 / (16.0 * g["TY"])))
    else:
        g, best = dict(E=1), -1.0
        for TX in range(8, 129):
            TY = 256 // TX
            if TX * TY < 192 or TY < 2:
                continue
            chunks, tiles = chunks_for(nx, TX), chunks_for(ny, TY)
            util = (nx / (chunks * TX)) * (ny / (tiles * TY))
            score = util + 0.05 + ((0.04 + 0.0005 * TX) if TX & (TX - 1) == 0 else 0.0)
            if score > best:
                best = score
                g.update(TX=TX, TY=TY, chunks=chunks, tiles=tiles)
        R = 32
        while R > 8 and g["chunks"] * g["tiles"] * B * _cdiv(nelz, R) < 2048:
            R //= 2
        g["R"] = max(min(R, nelz), 1)
    g["strips"] = _cdiv(nelz, g["R"])
    return g


def plan3d_env(ngp, mesh, B, allow_e2, need_e2, override):
    g = plan3d(ngp, mesh, B, allow_e2)
    if override:
        try:
            TX, TY, E, R = (int(x) for x in override.split(","))
        except ValueError:
            return g
        if TX * TY >= 64 and (E == 1 or (E == 2 and allow_e2 and TX == 16 and TY == 16)) and R >= 1 and TX * TY <= 256 and \
                not (need_e2 and allow_e2 and E == 1):
            nx, ny, nz = mesh
            nelz = nz - 1
            g = dict(TX=TX, TY=TY, E=E, R=min(R, nelz), chunks=chunks_for((nx - 1) // E + 1, TX), tiles=chunks_for(ny, TY))
            g["strips"] = _cdiv(nelz, g["R"])
    return g


def _is_field(x):
    return isinstance(x, np.ndarray)


def choose(c, plan=None, switches=None, strip_select=0):
    """poisson_choose for a 3-D Q1 argument set (every array 16-byte aligned): (family name | None when the call is refused, geometry)"""
    plan = c["plan"] if plan is None else plan
    sw = c["switches"] if switches is None else switches
    ngp, (nx, ny, nz) = c["ngp"], c["mesh"]
    w = c["tables"][2]
    imgs = [m for m in c["conds"] if m["kind"] != "box"]
    box = any(m["kind"] == "box" for m in c["conds"])
    kinds = {m["kind"] for m in imgs}
    n2_ok = ngp == 2 and nx % 2 == 0 and c["fkind"] != "gp" and w[0] == 1.0 and w[1] == 1.0 and \
        not any(_is_field(m["value"]) for m in imgs) and len(kinds) < 2
    t16 = bool(sw.get("Q1_3D_T16"))
    e2 = n2_ok and not t16 and not sw.get("Q1_3D_E1")
    if (box or c["fkind"] == "load") and not e2:
        return None, None
    g = plan3d_env(ngp, c["mesh"], c["B"], e2, box or c["fkind"] == "load", plan)
    if g["E"] == 2:
        Bt = c["tables"][0]
        kap = [np.float32(c["alpha"]) * np.float32(c["wscale"]) * np.float32(1.0 / h) ** 2 for h in HS]
        cfz = not sw.get("Q1_3D_N2") and not sw.get("Q1_3D_E1SUM") and c["alpha"] != 0.0 and all(k != 0 for k in kap) and \
            not abs(np.float32(Bt[0, 1] + Bt[1, 1]) - np.float32(1.0)) > 1e-6
        fam = "cfz" if cfz else "n2"
    else:
        u8c = all(m["kind"] == "u8" and not _is_field(m["value"]) for m in imgs)
        f32c = all(m["kind"] == "f32" and not _is_field(m["value"]) for m in imgs)
        owner = g["TX"] == 16 and g["TY"] == 16 and not t16 and c["fkind"] != "gp" and (not imgs or u8c or f32c)
        fam = "n1" if owner else ("t16" if g["TX"] == 16 else "generic")
    g = dict(g, launched_strips=min(g["strips"], 2) if strip_select == 1 else (max(g["strips"] - 2, 0) if strip_select == 2 else g["strips"]))
    g["launched"] = g["chunks"] * g["tiles"] * g["launched_strips"] * c["B"]
    return fam, g


def selectors(c):
    """the kernel template and its arguments as the host picks them: (template, NGP, frozenset of flag names[, UW]) -- from poisson_choose down
    to the hipLaunchKernelGGL line"""
    fam, g = choose(c)
    ngp, sw = c["ngp"], c["switches"]
    imgs = [m for m in c["conds"] if m["kind"] != "box"]
    box = any(m["kind"] == "box" for m in c["conds"])
    unit = all(x == 1.0 for x in c["tables"][2])
    fl = set()
    if c["nu"] is not None:
        fl.add("NU")
    e1g = c["alpha"] != 0.0 and c["want_sums"] and not sw.get("Q1_3D_E1SUM")
    if fam in ("cfz", "n2"):
        if c["fkind"] in ("nodal", "load"):
            fl.add("F")
        if c["fkind"] == "load":
            fl.add("LOAD")
        if fam == "n2" and e1g:
            fl.add("E1G")
        f32 = any(m["kind"] == "f32" for m in imgs)
        if box:
            fl.add("BOX")
            if imgs:
                fl |= {"IMG", "ONE"} | ({"F32"} if f32 else set())
        elif imgs:
            fl |= {"IMG"} | ({"ONE"} if len(imgs) == 1 else set()) | ({"F32"} if f32 else set())
        return (fam, 2, frozenset(fl))
    if c["fkind"] == "nodal":
        fl.add("F")
    if c["fkind"] == "gp":
        fl.add("FGP")
    u8c = bool(imgs) and all(m["kind"] == "u8" and not _is_field(m["value"]) for m in imgs)
    f32c = bool(imgs) and all(m["kind"] == "f32" and not _is_field(m["value"]) for m in imgs)
    uw = ngp == 2 and unit
    if fam == "n1":
        if imgs and u8c:
            fl.add("U8C")
        elif imgs:                               # launch3_f32n: no FL3_E1G instantiation exists for fp32 images
            assert f32c
            fl |= {"U8C", "F32"}
        if imgs and len(imgs) == 1:
            fl.add("ONE")
        if uw and e1g and "F32" not in fl:
            fl.add("E1G")
        return ("n1", ngp, frozenset(fl), uw)
    if imgs:
        fl.add("U8C" if u8c else "BC")
    return (fam, ngp, frozenset(fl), uw)


def expected_kernels(family, ngp):
    """the instantiations behind the launch functions, written down as the full product (independently of `selectors`)"""
    def fs(*parts):
        return frozenset(x for p in parts for x in p)
    if family in ("cfz", "n2"):
        if ngp != 2:
            return set()
        bases = [(), ("NU",), ("F",), ("NU", "F"), ("F", "LOAD"), ("NU", "F", "LOAD")]
        conds = [(), ("IMG", "ONE"), ("IMG",), ("IMG", "F32", "ONE"), ("IMG", "F32"), ("BOX",), ("BOX", "IMG", "ONE"), ("BOX", "IMG", "F32", "ONE")]
        e1 = [(), ("E1G",)] if family == "n2" else [()]
        return {(family, 2, fs(b, k, e)) for b in bases for k in conds for e in e1}
    bases = [(), ("NU",), ("F",), ("NU", "F")]
    if family == "n1":
        u8, f32 = [(), ("U8C",), ("U8C", "ONE")], [("U8C", "F32"), ("U8C", "F32", "ONE")]
        out = {("n1", ngp, fs(b, k), False) for b in bases for k in u8 + f32}
        if ngp == 2:
            out |= {("n1", 2, fs(b, k, e), True) for b in bases for k in u8 for e in [(), ("E1G",)]}
            out |= {("n1", 2, fs(b, k), True) for b in bases for k in f32}
        return out
    bases += [("FGP",), ("NU", "FGP")]
    return {(family, ngp, fs(b, k), uw) for b in bases for k in [(), ("U8C",), ("BC",)] for uw in ([False, True] if ngp == 2 else [False])}


# ---------------------------------------------------------------------------------------------
# seeded data
# ---------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def rnd(shape, *key, lo=-0.5, width=1.0):
    return (lo + width * _rng(*key).random(shape)).astype(np.float32)


def seam_lines(mesh, g):
    """(columns, rows, planes): the node lines on both sides of every chunk, tile and strip seam of a geometry, plus the last of each"""
    nx, ny, nz = mesh
    cx, cy = g["E"] * (g["TX"] - 1), g["TY"] - 1            # columns / rows a workgroup owns
    cols = {k * cx + d for k in range(1, g["chunks"]) for d in (-1, 0, 1)} | {nx - 1}
    rows = {k * cy + d for k in range(1, g["tiles"]) for d in (-1, 0, 1)} | {ny - 1}
    planes = {k * g["R"] + d for k in range(1, g["strips"]) for d in (-1, 0, 1)} | {nz - 1}
    return tuple(sorted(x for x in s if 0 <= x < n) for s, n in ((cols, nx), (rows, ny), (planes, nz)))


def mask_image(mesh, Bm, kind, lines, *key):
    """(Bm, nz, ny, nx): a 20 % blob per sample; on every seam line (and the last column, row and plane) one node of four fixed and one of four free
    along the other two axes; the eight corners alternately fixed and free.  "u8": 0 / 1 / 255; "f32": 0 / 1, a tenth of the nodes taking
    exactly 0.5 or one of its two float32 neighbours (0.5 and the one below are free under dn_dirichlet)."""
    nx, ny, nz = mesh
    rs = _rng("mask", *key)
    m = rs.random((Bm, nz, ny, nx)) < 0.2
    off = int(_rng("offset", *key[:-1]).integers(0, 12))
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ph = (x + y + z + off) % 4
    cols, rows, planes = lines
    on = np.isin(x, cols) | np.isin(y, rows) | np.isin(z, planes)
    m[:, on & (ph == 0)] = True
    m[:, on & (ph == 2)] = False
    for k, (cz, cy, cx) in enumerate(itertools.product((0, nz - 1), (0, ny - 1), (0, nx - 1))):
        m[:, cz, cy, cx] = (k + off) % 2 == 0
    if kind == "u8":
        return np.where(m, np.where(rs.random(m.shape) < 0.5, 255, 1), 0).astype(np.uint8)
    img = m.astype(np.float32)
    half = np.float32(0.5)
    edge = np.array([half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1))], dtype=np.float32)
    pick_ = rs.random(m.shape) < 0.1
    return np.where(pick_, edge[rs.integers(0, 3, m.shape)], img).astype(np.float32)


def box_image(mesh, faces):
    nx, ny, nz = mesh
    m = np.zeros((nz, ny, nx), bool)
    for bit, idx in ((1, np.s_[:, :, 0]), (2, np.s_[:, :, -1]), (4, np.s_[:, 0]), (8, np.s_[:, -1]), (16, np.s_[0]), (32, np.s_[-1])):
        if faces & bit:
            m[idx] = True
    return m


def fixed_nodes(cond, mesh, b, ge=False):
    """the Dirichlet nodes of one condition for sample b: uint8 != 0, fp32 > 0.5 (dn_dirichlet), the named box faces.  ge: the wrong `>=`"""
    if cond["kind"] == "box":
        return box_image(mesh, cond["faces"])
    m = pick(cond["img"], b)
    if m.dtype == np.uint8:
        return m != 0
    return (m >= np.float32(0.5)) if ge else (m > np.float32(0.5))


def pick(a, b):
    return a[b if a.shape[0] > 1 else 0] if isinstance(a, np.ndarray) else a


def rule_points(rule):
    if RULES[rule] is None:
        from diffnet_amd.tables import gauss_rule
        gx, gw = gauss_rule(NGP[rule])
        return np.asarray(gx, float), np.asarray(gw, float)
    return tuple(np.asarray(t, float) for t in RULES[rule])


@functools.lru_cache(maxsize=None)
def tables(rule):
    """(N, dN, w) as dn_mesh carries them (FemGeometry.mesh_struct): float32"""
    from diffnet_amd.tables import Basis1D
    gx, gw = rule_points(rule)
    Bv, Dv, _ = Basis1D(1).at_gauss(gx)
    return tuple(np.asarray(t, dtype=np.float32) for t in (Bv, Dv, gw))


# ---------------------------------------------------------------------------------------------
# the argument sets
# ---------------------------------------------------------------------------------------------
def _cond_list(cond, i, flip=False):
    """kinds of the conditions in order; "val": a uint8 image with a value field; the box comes second with flip"""
    if cond == "none":
        return []
    if cond in ("u8x1", "u8x2", "f32x1", "f32x2"):
        return [cond[:-2]] * int(cond[-1])
    if cond == "box":
        return ["box"]
    if cond in ("box+u8", "box+f32"):
        k = [cond[4:], "box"]
        return k[::-1] if flip else k
    if cond == "u8c":
        return ["u8"] * (1 + i % 2)
    if cond == "general":
        return [["val", "u8"], ["u8", "f32"], ["f32", "valf"], ["val"]][i % 4]
    raise ValueError(cond)


@functools.lru_cache(maxsize=None)
def build(case):
    """the argument set of a case: numpy float32 / uint8 arrays and Python floats"""
    family, rule, base, cond, mesh, B, plan, route, i = case
    nx, ny, nz = mesh
    key = (family, rule, base, cond, mesh, B, plan, i)          # the data do not depend on the route: two routes of one i share their arguments
    ngp = NGP[rule]
    shape = (nz, ny, nx)
    c = dict(case=case, family=family, rule=rule, ngp=ngp, mesh=mesh, B=B, plan=plan, shape=shape, tables=tables(rule), **CONST)
    sw = {}
    if "e1" in route.split("+"):
        sw["Q1_3D_E1"] = "1"
    if "t16" in route.split("+"):
        sw["Q1_3D_T16"] = "1"
    if "n2" in route.split("+"):
        sw["Q1_3D_N2"] = "1"
    if "e1sum" in route.split("+"):
        sw["Q1_3D_E1SUM"] = "1"
    if "alpha0" in route.split("+"):
        c["alpha"] = 0.0
    c["switches"], c["want_sums"] = sw, "nosums" not in route.split("+")
    if "offset" in route.split("+"):
        c["u"] = (np.float32(8.0) + rnd((B, *shape), *key, "u") / np.float32(8.0)).astype(np.float32)
    else:
        c["u"] = rnd((B, *shape), *key, "u", lo=-1.0, width=2.0)
    c["nu"] = rnd((B if i % 2 == 0 else 1, *shape), *key, "nu", lo=0.5) if "N" in base else None
    fb = B if (i // 2) % 2 == 0 else 1
    c["fkind"], c["f"] = None, None
    if "G" in base:
        c["fkind"], c["f"] = "gp", rnd((fb, ngp ** 3, nz - 1, ny - 1, nx - 1), *key, "fgp", lo=-2.0, width=4.0)
    elif "F" in base:
        c["fkind"], c["f"] = "nodal", rnd((fb, *shape), *key, "f", lo=-2.0, width=4.0)
    # the conditions; their masks carry the seam pattern of the geometry the launch will have
    kinds = _cond_list(cond, i, len(base) % 2 == 1)
    c["conds"] = [dict(kind={"val": "u8", "valf": "f32"}.get(k, k), value=0.0) for k in kinds]
    vals = (0.3125, -0.25)
    for k, m in enumerate(c["conds"]):
        m["value"] = vals[k]
        if kinds[k] in ("val", "valf"):
            m["value"] = rnd((B if (i + k) % 2 else 1, *shape), *key, "val", k)
        if m["kind"] == "box":
            m["faces"] = 63 if "F" not in base else (FACES["xlo"] | FACES["yhi"] | FACES["zhi"])
    if "L" in base:
        c["fkind"] = "load"
    _, g = choose(c)
    assert g is not None, case
    lines = seam_lines(mesh, g)
    for k, m in enumerate(c["conds"]):
        if m["kind"] != "box":
            m["img"] = mask_image(mesh, B if (i + k) % 2 == 0 else 1, m["kind"], lines, *key, k)
    if "L" in base:                      # b_a = sum_e sum_g w_g N_a(g) f_g of the nodal forcing, in float64, stored as float32
        t = c["tables"]
        c["f"] = np.stack([poisson3d(np.zeros(shape, np.float32), None, c["f"][b], "nodal", [], [], t, alpha=0.0, beta=-1.0, c=0.0, wscale=1.0,
                                     out_scale=1.0)["out"] for b in range(c["f"].shape[0])]).astype(np.float32)
    return c


BASES_N = ["", "N", "F", "NF"]
BASES_E2 = BASES_N + ["FL", "NFL"]
BASES_W = BASES_N + ["G", "NG"]
CONDS_E2 = ["none", "u8x1", "u8x2", "f32x1", "f32x2", "box", "box+u8", "box+f32"]
CONDS_N1 = ["none", "u8x2", "u8x1", "f32x2", "f32x1"]
CONDS_W = ["none", "u8c", "general"]


def part1_cases(family):
    """the matrix of one family (module docstring of test_gpu_poisson3d_forms.py), on the part-1 meshes with B = 2"""
    out, plan = [], PLAN1[family]
    add = lambda rule, base, cond, mesh, route: out.append(Case(family, rule, base, cond, mesh, 2, plan, route, len(out)))       # noqa: E731
    if family == "cfz":
        for base, cond in itertools.product(BASES_E2, CONDS_E2):
            add("g2", base, cond, MESH_E, "sums")
    elif family == "n2":
        for n, (base, cond) in enumerate(itertools.product(BASES_E2, CONDS_E2)):
            n += n // 8                                                                                      # (rotate against the 8 conditions)
            add(("g2", "u2")[n % 2], base, cond, MESH_E, ("n2", "sums")[n % 2])                              # FL3_E1G on: by the switch, by the rule
            add(("u2", "g2", "g2", "g2")[n % 4], base, cond, MESH_E, ("nosums", "n2+nosums", "alpha0", "e1sum")[n % 4])       # FL3_E1G off
    elif family == "n1":
        for rule, route in (("g2", "sums"), ("g2", None), ("w2", "sums"), ("g3", "sums"), ("g4", "sums")):
            for base, cond in itertools.product(BASES_N, CONDS_N1):
                n = len(out)
                mesh = (MESH_E, MESH_O)[n % 2]
                r = route if route else ("nosums", "alpha0", "e1sum")[n % 3]
                add(rule, base, cond, mesh, r + ("+e1" if rule in ("g2", "u2") and mesh == MESH_E else ""))
    else:
        for rule in ("g2", "w2", "g3", "g4"):
            for base, cond in itertools.product(BASES_W, CONDS_W):
                add(rule, base, cond, (MESH_E, MESH_O)[len(out) % 2], "sums")
    return out


# part 2: (mesh, B, rule, plan override, route, base, cond); what each reaches is asserted by test_seam_list_reaches_every_seam
SEAMS = [
    # two-element forms on the default plan, the closed form in z and (switch) the per-point kernel
    ((2, 2, 2), 1, "g2", "", "sums", "NF", "u8x2"), ((32, 16, 2), 1, "g2", "", "sums", "NF", "f32x2"), ((32, 16, 3), 2, "g2", "", "sums", "NF", "box+u8"),
    ((34, 17, 6), 1, "g2", "", "sums", "NFL", "u8x2"), ((62, 16, 6), 1, "g2", "", "sums", "NF", "u8x1"), ((64, 17, 6), 1, "g2", "", "sums", "F", "f32x1"),
    ((34, 17, 6), 2, "g2", "16,16,2,1", "sums", "NF", "u8x2"), ((34, 17, 6), 1, "g2", "16,16,2,2", "sums", "N", "box"),
    ((2, 2, 2), 1, "g2", "", "n2", "NF", "u8x2"), ((32, 16, 2), 1, "g2", "", "n2", "NF", "f32x2"), ((32, 16, 3), 2, "g2", "", "n2", "NF", "box+u8"),
    ((34, 17, 6), 1, "g2", "", "n2", "NFL", "u8x2"), ((62, 16, 6), 1, "g2", "", "n2", "NF", "u8x1"), ((64, 17, 6), 1, "g2", "", "n2", "F", "f32x1"),
    ((34, 17, 6), 2, "g2", "16,16,2,1", "n2", "NF", "u8x2"), ((34, 17, 6), 1, "g2", "16,16,2,2", "n2", "N", "box"),
    # one-element forms on the default plan: node-owner form at 16 x 16 tiles, T16 tile heights 4, 8, 12, the generic form
    ((16, 16, 5), 1, "g2", "", "sums+e1", "NF", "u8x2"), ((17, 16, 5), 2, "g2", "", "sums", "NF", "f32x2"), ((31, 16, 5), 1, "g2", "", "sums", "NF", "u8x1"),
    ((17, 17, 5), 3, "g2", "", "sums", "NG", "general"), ((31, 31, 5), 3, "g2", "", "sums", "NF", "u8c"), ((17, 4, 5), 1, "g2", "", "sums", "NG", "general"),
    ((17, 8, 5), 3, "w2", "", "sums", "NF", "u8c"), ((16, 31, 5), 1, "g2", "", "sums+t16", "NF", "general"), ((16, 16, 5), 1, "g3", "", "sums", "NF", "u8x2"),
    ((17, 17, 5), 1, "g4", "", "sums", "NF", "f32x2"), ((31, 31, 11), 1, "g3", "", "sums", "NG", "general"), ((23, 11, 5), 1, "g3", "", "sums", "NG", "general"),
    ((2, 2, 2), 1, "g3", "", "sums", "NF", "u8x2"), ((31, 16, 5), 1, "w2", "16,16,1,1", "sums", "NF", "u8x2"),
]


def part2_cases():
    return [Case("seam", rule, base, cond, mesh, B, plan, route, 500 + k) for k, (mesh, B, rule, plan, route, base, cond) in enumerate(SEAMS)]


def offset_cases():
    """u = 8 + rnd / 8 on the closed form in z and on a Q1_3D_E1SUM launch of the same arguments (the per-point two-element kernel)"""
    return [Case("offset", "g2", "NF", "none", MESH_E, 2, "16,16,2,3", r, 900) for r in ("sums+offset", "e1sum+offset")]


def all_cases():
    return [c for f in FAMILIES for c in part1_cases(f)] + part2_cases()


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
def poisson3d(u, nu, f, fkind, fixed, vals, tabs, alpha, beta, c, wscale, out_scale, *, dtype=np.float64, scale=False, hs=HS, load_twice=False):
    """dn_poisson_apply on one sample of a 3-D Q1 mesh, or on a batch of them (any leading axes; the scalars are then the totals).  u, nu
    (or None), f: (nz, ny, nx) float32 (f at Gauss points: (G, nelz, nely, nelx),
    x fastest in G; load vector: nodal b); fixed / vals: the conditions in order (boolean images; constants or nodal fields).  Every
    operation is done in `dtype`.  Returns a dict: out, E1, E2, energy, sumsq, fixed (the union), ut (u~), and with scale=True S, SE1, SE2, SN."""
    dt = dtype
    N, dN, w = (np.asarray(t, dtype=np.float32).astype(dt) for t in tabs)
    ngp = len(w)
    sc = [dt(2.0) / dt(h) for h in hs]
    alpha, beta, c, wscale, out_scale = (dt(np.float32(x)) for x in (alpha, beta, c, wscale, out_scale))
    ut = u.astype(dt)
    fx = np.zeros(u.shape, bool)
    for m, v in zip(fixed, vals):
        ut = np.where(m, np.asarray(v, dtype=np.float32).astype(dt), ut)
        fx = fx | m
    nz, ny, nx = u.shape[-3:]
    corners = list(itertools.product((0, 1), repeat=3))                   # (kz, ky, kx)
    sl = {k: np.s_[..., k[0]:nz - 1 + k[0], k[1]:ny - 1 + k[1], k[2]:nx - 1 + k[2]] for k in corners}
    Uc = {k: np.ascontiguousarray(ut[sl[k]]) for k in corners}
    NUc = None if nu is None else {k: np.ascontiguousarray(nu.astype(dt)[sl[k]]) for k in corners}
    Fc = {k: np.ascontiguousarray(f.astype(dt)[sl[k]]) for k in corners} if fkind == "nodal" else None
    out = np.zeros(u.shape, dt)
    S = np.zeros(u.shape, dt) if scale else None
    E1 = E2 = SE1 = SE2 = dt(0)
    for gz, gy, gx in itertools.product(range(ngp), repeat=3):
        W = w[gx] * w[gy] * w[gz] * wscale
        Nc = {k: N[gx, k[2]] * N[gy, k[1]] * N[gz, k[0]] for k in corners}
        D = [{k: dN[gx, k[2]] * sc[0] * N[gy, k[1]] * N[gz, k[0]] for k in corners},
             {k: N[gx, k[2]] * dN[gy, k[1]] * sc[1] * N[gz, k[0]] for k in corners},
             {k: N[gx, k[2]] * N[gy, k[1]] * dN[gz, k[0]] * sc[2] for k in corners}]
        ug = sum(Nc[k] * Uc[k] for k in corners)
        grad = [sum(Dd[k] * Uc[k] for k in corners) for Dd in D]
        nug = dt(1) if nu is None else sum(Nc[k] * NUc[k] for k in corners)
        if fkind == "nodal":
            fg = sum(Nc[k] * Fc[k] for k in corners)
        elif fkind == "gp":
            fg = f[..., (gz * ngp + gy) * ngp + gx, :, :, :].astype(dt)
        else:
            fg = None
        e1 = W * nug * (grad[0] * grad[0] + grad[1] * grad[1] + grad[2] * grad[2])
        E1 = E1 + e1.sum(dtype=dt)
        if fg is not None:
            E2 = E2 + (W * ug * fg).sum(dtype=dt)
        if scale:
            SE1 = SE1 + np.abs(e1).sum(dtype=dt)
            if fg is not None:
                SE2 = SE2 + np.abs(W * ug * fg).sum(dtype=dt)
        for k in corners:
            t = W * alpha * nug * (D[0][k] * grad[0] + D[1][k] * grad[1] + D[2][k] * grad[2])
            if fg is not None:
                t = t - W * beta * Nc[k] * fg
            out[sl[k]] += t
            if scale:
                S[sl[k]] += np.abs(t)
    if fkind == "load":
        b = f.astype(dt) * (wscale if load_twice else dt(1))
        out = out - beta * wscale * b
        E2 = (wscale * ut * b).sum(dtype=dt)
        if scale:
            S = S + np.abs(beta * wscale * b)
            SE2 = (np.abs(wscale) * np.abs(ut * b)).sum(dtype=dt)
    res = dict(ut=ut, fixed=fx, E1=E1, E2=E2, energy=c * E1 - E2)
    if scale:
        res.update(S=S, SE1=SE1, SE2=SE2, SN=(np.abs(ut) * S).sum(dtype=dt))
    raw = np.where(fx, dt(0), out)
    res["sumsq"] = (raw * raw).sum(dtype=dt)
    res["raw"] = raw
    res["out"] = out_scale * raw
    assert res["out"].dtype == dt
    return res


def evaluate(c, *, dtype=np.float64, scale=False, mutate=None):
    """The restatement on every sample of an argument set.  Returns dict: out, S, fixed (B, nz, ny, nx); energy, sumsq, E1, E2, SE1, SE2, SN
    summed over the batch.  mutate: a deliberately wrong evaluation (test_comparator_has_teeth)."""
    B, mesh, tabs = c["B"], c["mesh"], c["tables"]
    kw = dict(alpha=c["alpha"], beta=c["beta"], c=c["c"], wscale=c["wscale"], out_scale=c["out_scale"], dtype=dtype, scale=scale)
    if mutate == "swap_xz":
        kw["hs"] = HS[::-1]
    if mutate == "weight":
        N, dN, w = tabs
        w = w.copy()
        w[1] = np.float32(w[1] * np.float32(1.0 + 2.0 ** -10))
        tabs = (N, dN, w)
    if mutate == "load_twice":
        assert c["fkind"] == "load"
        kw["load_twice"] = True
    full = lambda a: np.broadcast_to(a, (B, *a.shape[1:]))                     # noqa: E731
    fixed = [np.stack([fixed_nodes(m, mesh, b, ge=mutate == "ge") for b in range(B)]) for m in c["conds"]]
    vals = [full(m["value"]) if _is_field(m["value"]) else m["value"] for m in c["conds"]]
    if mutate == "order":
        fixed, vals = fixed[::-1], vals[::-1]
    nu = None if c["nu"] is None else full(c["nu"])
    if mutate == "nu_batched":           # a shared nu indexed per sample: sample b reads the memory b samples further on -- here another field
        assert c["nu"].shape[0] == 1 and B > 1
        nu = np.stack([nu[0]] + [(np.abs(c["u"][b - 1]) + np.float32(0.5)).astype(np.float32) for b in range(1, B)])
    f = None if c["f"] is None else full(c["f"])
    r = poisson3d(c["u"], nu, f, c["fkind"], fixed, vals, tabs, **kw)
    res = dict(out=r["out"], fixed=r["fixed"], raw=r["raw"])
    for n in ("energy", "sumsq", "E1", "E2") + (("SE1", "SE2", "SN") if scale else ()):
        res[n] = float(r[n])
    if scale:
        res["S"] = r["S"]
        res["ref_raw_abs_S"] = float((np.abs(r["raw"]) * np.where(r["fixed"], 0.0, r["S"])).sum())
    return res


@functools.lru_cache(maxsize=None)
def reference(case):
    """float64 values and scales of a case: computed once per session and left unchanged"""
    r = evaluate(build(case), scale=True)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


# ---------------------------------------------------------------------------------------------
# the comparator and the bounds
# ---------------------------------------------------------------------------------------------
def node_error(got, ref, out_scale):
    """e = |got - ref64| / (|out_scale| S_a) per node; inf where a rule is broken: a non-finite value, a free node without a term that is not
    exactly 0, a Dirichlet node that is not exactly 0.  Returns (max e, its index)."""
    got = np.asarray(got).astype(np.float64)
    r, S, fixed = ref["out"].astype(np.float64), np.abs(out_scale) * ref["S"].astype(np.float64), ref["fixed"]
    assert got.shape == r.shape, (got.shape, r.shape)
    pos = S > 0
    e = np.where(pos, np.abs(got - r) / np.where(pos, S, 1.0), np.where(got == 0.0, 0.0, math.inf))
    e = np.where(fixed, np.where(got == 0.0, 0.0, math.inf), e)
    e = np.where(np.isfinite(got), e, math.inf)
    at = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[at]), tuple(int(x) for x in at)


def forcing_form(c):
    return {None: "absent", "nodal": "nodal", "gp": "gp", "load": "load"}[c["fkind"]]


@functools.lru_cache(maxsize=None)
def yardsticks():
    """Y per (points of the rule, forcing form): the largest e of the float32 evaluation of the restatement over every case of the file"""
    Y = {}
    for case in all_cases():
        c = build(case)
        e, at = node_error(evaluate(c, dtype=np.float32)["out"], reference(case), c["out_scale"])
        assert math.isfinite(e), (case, at)
        k = (c["ngp"], forcing_form(c))
        if e > Y.get(k, (0.0, None))[0]:
            Y[k] = (e, case)
    return Y


def K_of(c):
    return MARGIN * yardsticks()[(c["ngp"], forcing_form(c))][0]


def chain_length(c, g, fam):
    """n of the scalar bounds n 2^-24 SE: the longest chain of float32 roundings between a placed product and the per-thread partial sum that
    leaves for the float64 reduction (finish_sums) -- the R layers of a strip (one fmaf each into e1_acc / e2_acc: `layer` in
    poisson3d_q1w_kernel, poisson3d_q1n_kernel, poisson3d_q1n2_kernel; `e2_acc += cs.x + cs.y` per layer in poisson3d_q1_cf_kernel), 2 for the
    two elements / lanes of a thread added at the end, the points of an element (q1_layer_3d_w sums ngp^3 point terms; the closed form's mass
    stencil 27 node terms) and 16 for the roundings inside one term (three sum-factorised stages for u, nu, f and each gradient component,
    the squares, their sum and the two weights)"""
    return g["R"] + 2 + (27 if fam == "cfz" else c["ngp"] ** 3) + 16


def scalar_bounds(c, ref, g, fam, nodal_e1):
    """(bound of |energy - ref|, bound of |sumsq - ref|).
    Per-point forms: |E1 err| <= n U SE1, |E2 err| <= n U SE2.
    Nodal-value forms (3d_q1_cfz, FL3_E1G): the thread forms e1 = ((sum_a u~_a t_a) / esc + beta e2) / alpha over its own nodes, t_a the node's
    value BEFORE the Dirichlet rows are zeroed.  t_a is within K S_a of float64 (the node bound), the products u~_a t_a are added in float32
    over the R + 1 planes of a strip (two lanes: + 1), and the identity sum_a u~_a t_a = alpha E1 - beta E2 (wscale inside S, SE) holds for
    the total; the two divisions and the fma cost 3 roundings of each operand's magnitude.  So
        |E1 err| <= ((K + (R + 5) U) SN + |beta| (n + 3) U SE2) / |alpha|.
    Load vector: E2 = wscale sum_a u~_a b_a, one fmaf per plane: (R + 4) U SE2.
    sumsq (sums_bound of q1_residual_ref.py, t^2 added per thread over the R + 1 planes of a strip, two lanes):
        2 K sum |raw64| S + (R + 4) U sumsq64."""
    n, R, K = chain_length(c, g, fam), g["R"], K_of(c)
    e2 = ((R + 4) if c["fkind"] == "load" else n) * U * ref["SE2"]
    if nodal_e1:
        e1 = ((K + (R + 5) * U) * ref["SN"] + abs(c["beta"]) * (e2 + 3 * U * ref["SE2"])) / abs(c["alpha"])
    else:
        e1 = n * U * ref["SE1"]
    return abs(c["c"]) * e1 + e2, 2.0 * K * ref["ref_raw_abs_S"] + (R + 4) * U * ref["sumsq"]
